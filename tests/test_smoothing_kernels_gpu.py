"""The two smoothing kernels of ``csrc/pf_smooth.hpp`` called directly - ``k_ffbs`` (``pf_smooth_ffbs``) and ``k_trace_ancestors``
(``pf_smooth_fixed_lag``) - against the float64 oracle, in both dtypes, on every built-in kind and at the shapes and weight edges
the kernels have code for (inputs and bars: ``tests/smoothing_cases.py``).

A backward draw is checked on its own: the oracle's step t is teacher-forced with the kernel's output at t + 1, so one differing
draw cannot move the later ones.  A draw that agrees with the float64 oracle is a bit-for-bit copy of that particle; one that
differs must lie within delta of every cdf boundary between the two picks, and at most 1e-3 of a case's draws may differ.
float64: delta = N 2^-52 x 8 (N additions in another order, a rescaling per new maximum).  float32: delta = 4 x the float32
oracle's own cdf error against the float64 oracle on the same inputs (the margin ``profiles/forecast.txt`` set for the forecast
kernel).  Measured figures: ``profiles/smoothing_parity.txt`` (the ``smoothing-parity:`` lines these tests print)."""
import ctypes as C
import math

import pytest
import torch

from oracle import cpu_ref
from oracle.cases import CASE_BY_NAME
from tests import smoothing_cases as sc
from tests.helpers import DT, build_filter_from_case, load_golden

pytestmark = pytest.mark.gpu


def _bits(t):
    """Bit pattern of a tensor (NaN-safe equality)."""
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def _run_ffbs(h, u=True, seed=3):
    from pyfilter_amd import ops

    kind, params = h.context()
    x_hist, logw, x_last, tape = h.soa()
    out = ops.smooth_ffbs(kind, params, x_hist, logw, x_last, tape if u else None, seed)
    torch.cuda.synchronize()
    return h.from_soa(out)


def _check_against_oracle(h, out, label):
    """Every backward draw of ``out (S, N, B, [D])`` over the history ``h`` against the float64 oracle; returns the oracle pass."""
    assert torch.equal(_bits(out[-1]), _bits(h.x_last)), f"{label}: the start of the backward pass is not x_last"
    nxt = lambda t: out[t]  # noqa: E731
    ref = sc.oracle_pass(h, torch.float64, x_next_of=nxt)
    if h.dtype == torch.float32:
        delta = sc.f32_delta(sc.oracle_pass(h, torch.float32, x_next_of=nxt), ref, 4.0)
    else:
        delta = sc.f64_delta(h.n)
    picks = [sc.recover_picks(h.x[t], out[t], prefer=ref["idx"][t]) for t in range(h.s - 1)]
    bad, total, worst = sc.compare_draws(h, picks, ref, delta, label)
    print(f"smoothing-parity: {label} {str(h.dtype)[6:]}: {bad} of {total} draws differ, largest boundary distance {worst:.3e}, delta {delta:.3e}")
    return ref, picks  # (``picks`` are exact matches: every row written is a bit-for-bit copy of the particle it names)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("model,n,b,s", sc.DRAW_CASES, ids=[f"{m}-{n}x{b}x{s}" for m, n, b, s in sc.DRAW_CASES])
def test_ffbs_every_draw_against_the_oracle(model, n, b, s, dt):
    h = sc.synthetic(model, n, b, s, DT[dt])
    label = f"{model} {n}x{b}x{s}"
    if s > 1:
        _check_against_oracle(h, _run_ffbs(h), label)
        return
    # S = 1: the output is x_last bit for bit and nothing else is written (a buffer twice the size, its tail a sentinel)
    from pyfilter_amd import _lib as L, ops

    kind, params = h.context()
    x_hist, logw, x_last, _ = h.soa()
    out = torch.full((2,) + tuple(x_hist.shape), -77.0, dtype=h.dtype, device="cuda")
    m = ops.make_model_struct(kind, params)
    L.check(L.load().pf_smooth_ffbs(C.byref(m), x_hist.data_ptr(), logw.data_ptr(), x_last.data_ptr(), None, 3, out.data_ptr(), 1, n, b,
                                    L.dtype_code(h.dtype), L.stream_ptr()), "pf_smooth_ffbs")
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[0, 0]), _bits(x_last))
    assert bool((out[1] == -77.0).all())
    assert torch.equal(_bits(_run_ffbs(h)[0]), _bits(h.x_last))


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("model,n,b,s", sc.EDGE_CASES, ids=[f"{m}-{n}x{b}x{s}" for m, n, b, s in sc.EDGE_CASES])
def test_ffbs_weight_and_offset_edges(model, n, b, s, dt):
    """A whole staged tile without mass (state 1, candidates 256..511); NaN, +inf and the lowest finite value among state 0's
    weights and, in column 1, all of its mass on candidate N - 1; u = 0 (the first candidate of positive mass) and u = 1 - eps
    (the last one, through the fallback)."""
    h = sc.edge_history(model, n, b, s, DT[dt])
    out = _run_ffbs(h)
    ref, picks = _check_against_oracle(h, out, f"edges {model} {n}x{b}x{s}")
    for t in range(s - 1):
        dead = cpu_ref.ffbs_sanitize_logw(h.logw[t]) == -math.inf
        assert not bool(dead.gather(0, picks[t]).any()), f"state {t}: a candidate without mass was drawn"
    if b > 1:
        assert bool((picks[0][:, 1] == n - 1).all())
    assert bool((picks[0][:10, 0] >= 3).all())  # (u = 0 over three leading candidates without mass)
    assert bool((picks[1] < 256).logical_or(picks[1] >= 512).all())


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("model", ["sine", "rw2d"])
def test_ffbs_philox_draws_follow_the_oracle_distribution(model, dt):
    """``u == NULL``: every trajectory of a column starts from the same value, so its N first backward draws are independent
    draws from one categorical the oracle knows - a chi-square over 32 equal-mass bins of the oracle's cdf (31 degrees of freedom:
    P(chi2 > 90) ~ 1e-7; fixed seed).  Same seed: same bits; another seed, and the other column (counter b N + j): other picks."""
    n, b = 4096, 2
    base = sc.synthetic(model, n, 1, 2, DT[dt], seed=2)
    # both columns hold the same history (these models have one parameter set): only the Philox counter tells them apart
    both = lambda v: v.expand(v.shape[:1] + (b,) + v.shape[2:]).contiguous()  # noqa: E731
    h = sc.History(model, DT[dt], [both(x) for x in base.x], [both(w) for w in base.logw], both(base.x_last[:1].expand_as(base.x_last)),
                   both(base.u[0])[None])
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
        print(f"smoothing-parity: philox {model} {dt} column {c}: chi2 {chi2:.2f} over {int(live.sum())} bins")
        assert chi2 < 90.0, chi2
    assert not torch.equal(picks[:, 0], picks[:, 1])  # identical columns, draw counters b N + j


FL_SHAPES = [(1, 3), (255, 2), (257, 9), (1000, 1)]


def _fl_values(s, n, b, d, dtype, gen):
    x = torch.randn((s, n, b, d), generator=gen, dtype=torch.float64).to(dtype)
    flat = x.view(-1)
    special = torch.tensor([-0.0, math.nan, torch.finfo(dtype).tiny / 4], dtype=dtype)  # (-0.0, a NaN, a subnormal)
    pos = torch.randperm(flat.numel(), generator=gen)[:3] if flat.numel() >= 3 else torch.arange(flat.numel())
    flat[pos] = special[: pos.numel()]
    return x


def _fl_ancestors(pattern, s, n, b, gen):
    if pattern == "random":
        return torch.randint(n, (s, n, b), generator=gen)
    if pattern == "identity":
        return torch.arange(n).view(1, n, 1).expand(s, n, b).contiguous()
    if pattern == "zero":
        return torch.zeros((s, n, b), dtype=torch.int64)
    if pattern == "last":
        return torch.full((s, n, b), n - 1, dtype=torch.int64)
    return torch.stack([torch.stack([torch.randperm(n, generator=gen) for _ in range(b)], 1) for _ in range(s)], 0)


def _check_fixed_lag(s, n, b, d, dtype, gen):
    from pyfilter_amd import ops

    x = _fl_values(s, n, b, d, dtype, gen)
    x_hist = x.permute(0, 3, 2, 1).contiguous().cuda()  # (S, D, B, N)
    for pattern in ("random", "identity", "zero", "last", "permutation"):
        anc = _fl_ancestors(pattern, s, n, b, gen)
        assert int(anc.min()) >= 0 and int(anc.max()) < n
        out = ops.smooth_fixed_lag(x_hist, anc.permute(0, 2, 1).contiguous().to(torch.int32).cuda())
        torch.cuda.synchronize()
        ref = cpu_ref.smooth_fl(list(x.unbind(0)), list(anc.unbind(0)))  # (S, N, B, D)
        assert torch.equal(_bits(out.permute(0, 3, 2, 1).cpu()), _bits(ref)), f"{pattern} ancestors, D = {d}"


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("n,s", FL_SHAPES)
def test_fixed_lag_is_the_oracle_gather_chain(n, s, b, dt):
    """``pf_smooth_fixed_lag`` against ``cpu_ref.smooth_fl``, bit patterns (``-0.0``, a NaN and a subnormal among the values), for
    D in {1, 2, 3, 5, 8} and random / identity / all-0 / all-(N-1) / permutation ancestors."""
    gen = torch.Generator().manual_seed(100 * n + 10 * s + b)
    for d in (1, 2, 3, 5, 8):
        _check_fixed_lag(s, n, b, d, DT[dt], gen)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_fixed_lag_is_the_oracle_gather_chain_past_the_block_cap(dt):
    """N = 2^20 + 3: more particles than the capped grid has threads, so the kernel's grid-stride loop iterates."""
    _check_fixed_lag(2, (1 << 20) + 3, 1, 1, DT[dt], torch.Generator().manual_seed(4))


E2E = [("lg1d_apf_lgo", "f32"), ("sine_apf_lgo", "f32"), ("rw2d_apf_lgo", "f32"),
       ("ou_apf_boot_theta", "f64"), ("lorenz_s_apf_boot", "f64"), ("rw2d_theta_apf_lgo", "f64")]


def _fix_resampler(filt, u_last):
    from pyfilter_amd import resampling

    filt._resampler = lambda w, normalized=False: resampling.systematic(w, normalized=normalized, u=u_last.cuda())


@pytest.mark.parametrize("name,dt", E2E)
def test_smooth_on_float32_and_unvisited_kinds_end_to_end(name, dt):
    """``ParticleFilter.smooth(states, "ffbs")`` under a tape on the recorded states of a fused run: every backward draw as in
    ``test_ffbs_every_draw_against_the_oracle``, teacher-forced from the recorded states - the host side too (the history's ring
    views, the tape's ``(S - 1, N, B) -> (S - 1, B, N)`` permutation, ``to_soa`` of the start)."""
    from pyfilter_amd.filters.utils import batched_gather

    case, dtype = CASE_BY_NAME[name], DT[dt]
    g = load_golden(name, dt)
    n, b, t_len = case["N"], case["B"], g["y"].shape[0]
    filt = build_filter_from_case(case, g, dtype, "cuda", record_states=True)
    states = filt.batch_filter(g["y"].cuda(), bar=False).states
    gen = torch.Generator().manual_seed(17)
    u_back = torch.rand((t_len, n, b), generator=gen, dtype=torch.float64).to(dtype)
    u_last = torch.rand(b, generator=gen, dtype=torch.float64).to(dtype)
    _fix_resampler(filt, u_last)
    filt.set_smoothing_tape(u_back)
    sm = filt.smooth(states, "ffbs")
    start = batched_gather(states[-1].timeseries_state.value, filt._resampler(states[-1].weights), 0)
    torch.cuda.synchronize()
    sm, start = sm.cpu(), start.cpu()
    assert sm.shape[0] == t_len + 1 and torch.equal(_bits(sm[-1]), _bits(start))
    h = sc.History(case["model"], dtype, [s.timeseries_state.value.cpu() for s in states], [s.weights.cpu() for s in states], start, u_back)
    h.case = case  # (the fixture's own case: its model under its own name and proposal)
    _check_against_oracle(h, sm, name)


def test_ffbs_over_a_bounded_ring_is_ffbs_over_the_tail_of_a_full_history():
    """``record_states=4``: the backward pass over the ring's four states is the one over the last four states of a full
    history under the same tape, bit for bit."""
    case = CASE_BY_NAME["sine_sisr_lgo"]
    g = load_golden(case["name"], "f64")
    gen = torch.Generator().manual_seed(23)
    u_back = torch.rand((3, case["N"], case["B"]), generator=gen, dtype=torch.float64)
    u_last = torch.rand(case["B"], generator=gen, dtype=torch.float64)
    got = []
    for keep in (True, 4):
        filt = build_filter_from_case(case, g, torch.float64, "cuda", record_states=keep)
        states = list(filt.batch_filter(g["y"].cuda(), bar=False).states)[-4:]
        assert len(states) == 4
        _fix_resampler(filt, u_last)
        filt.set_smoothing_tape(u_back)
        got.append(filt.smooth(states, "ffbs").cpu())
    assert got[0].shape[0] == 4 and torch.equal(_bits(got[0]), _bits(got[1]))


def test_smoothing_entry_points_refuse_what_they_do_not_serve():
    """``PF_HID_LINEAR_MAT`` and ``PF_HID_USER_AFFINE`` models: ``PF_EUNSUPPORTED`` from ``pf_smooth_ffbs``; S = 0, N = 0, a null
    ``x_hist`` (and D = 0 for the fixed-lag smoother): ``PF_EINVAL`` - all before any launch: the output buffer is untouched."""
    from pyfilter_amd import _lib as L

    lib = L.load()
    EINVAL, EUNSUPPORTED = -1, -3  # include/pf_amd.h
    s, d, b, n = 3, 2, 2, 64
    dev = "cuda"
    x_hist = torch.randn((s, d, b, n), device=dev, dtype=torch.float64)
    logw = torch.randn((s, b, n), device=dev, dtype=torch.float64)
    x_last = torch.randn((d, b, n), device=dev, dtype=torch.float64)
    anc = torch.zeros((s, b, n), device=dev, dtype=torch.int32)
    params = torch.ones(256, device=dev, dtype=torch.float64)
    out = torch.full((s, d, b, n), -77.0, device=dev, dtype=torch.float64)

    def model(hid, dim=d, obs_dim=d):
        m = L.PfModel()
        m.hid_kind, m.obs_kind, m.dim, m.obs_dim, m.dt, m.inc_scale, m.params = hid, L.OBS_LINEAR, dim, obs_dim, 1.0, 1.0, params.data_ptr()
        return m

    def ffbs(m, x=x_hist, S=s, N=n):
        return lib.pf_smooth_ffbs(C.byref(m), L.ptr(x), logw.data_ptr(), x_last.data_ptr(), None, 1, out.data_ptr(), S, N, b, L.PF_F64,
                                  L.stream_ptr())

    def fl(x=x_hist, S=s, N=n, D=d):
        return lib.pf_smooth_fixed_lag(L.ptr(x), anc.data_ptr(), out.data_ptr(), S, N, b, D, L.PF_F64, L.stream_ptr())

    assert ffbs(model(L.HID_LINEAR_MAT)) == EUNSUPPORTED
    assert ffbs(model(L.HID_USER_AFFINE)) == EUNSUPPORTED
    rw = model(L.HID_LINEAR)
    assert ffbs(rw, S=0) == EINVAL and ffbs(rw, N=0) == EINVAL and ffbs(rw, x=None) == EINVAL
    assert fl(S=0) == EINVAL and fl(N=0) == EINVAL and fl(x=None) == EINVAL and fl(D=0) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == -77.0).all())
