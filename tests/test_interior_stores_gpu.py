"""The per-step route stores an interior state's log-weights and ancestors only where somebody reads them
(``FusedArgs::keep_state``, ``pf_fused.hpp: step_body`` stage 4; the rule: ``pf_step.hip: filter_run_impl``).

* An APF step names new ancestors at every move, and the APF step after an observed one always resamples (apf.py:29-31) from the
  tile partials and the scans - it never loads the incoming log-weights.  Without a state history the log-weights are double
  buffered and there is one ancestor buffer, so on an interior observed -> observed APF step both planes would be overwritten
  unread: they are not stored.  The LAST step of every ``pf_filter_run`` call and every recorded state (``ring >= 3``) keep all
  four planes.
* A following unobserved step carries the weights and reads them; SISR keeps its ancestors across the steps that do not
  resample: those keep every store.

``test_interior_log_weights_are_not_stored`` looks at the buffers (a sentinel survives where the stores are gone).  The other
tests compare a one-piece run - interior steps - with the same run issued move by move - every step the last of its call, so
every plane stored - on the same seed and epoch.  What the rule can touch is the STATE: particles, log-weights and ancestors
are compared bit for bit.  Moment rows and log-likelihoods are compared to 1e-9 relative: a piece starts with
``k_fused_reduce``, whose partials are summed in another order than the step kernel's own, and takes its moments about another
pivot (``FusedArgs::pivot``: the run's record instead of the mean two states back), so these differ in rounding between a
one-piece and a piecewise run whatever is stored (the bar of ``tests/test_filters_gpu.py`` for float64 runs)."""
import ctypes as C

import pytest
import torch

from oracle.cases import build_spec, simulate
from pyfilter_amd import _lib as L, ops
from pyfilter_amd.hints import HINTS
from tests.helpers import build_ssm_from_case

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


@pytest.fixture(autouse=True)
def _per_step_route(monkeypatch):
    """The rule lives on the per-step route (the column / cluster kernels write a run's state once)."""
    monkeypatch.setattr(HINTS, "route", 1)


def _case(model, filt_name, prop, n, b, t_len, ess=0.9, nan_steps=()):
    return dict(name=f"{model}_{filt_name}_{prop}", model=model, filter=filt_name, proposal=prop, N=n, B=b, T=t_len,
                ess_threshold=ess, seed=4242, nan_steps=tuple(nan_steps))


def _filter(case, dtype, seed=31, **kwargs):
    from pyfilter_amd.filters.particle import APF, SISR, proposals

    ssm = build_ssm_from_case(case, dtype, "cuda")
    prop = {"bootstrap": proposals.Bootstrap, "lgo": proposals.LinearGaussianObservations}[case["proposal"]]()
    filt = {"sisr": SISR, "apf": APF}[case["filter"]](ssm, case["N"], proposal=prop, ess_threshold=case["ess_threshold"], seed=seed, **kwargs)
    filt.set_batch_shape(torch.Size([case["B"]]))
    return filt


def _observations(case, dtype):
    return simulate(case, build_spec(case, F64)).to(dtype).cuda()


def _bits(t):
    """Bit pattern of a tensor (NaN-safe equality)."""
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def _same_state(a, b, what):
    """Particles, log-weights and ancestors of two ``ParticleFilterCorrection``s, bit for bit."""
    assert torch.equal(a.previous_indices, b.previous_indices), f"{what}: ancestors differ"
    assert torch.equal(_bits(a.weights), _bits(b.weights)), f"{what}: log-weights differ"
    assert torch.equal(_bits(a.timeseries_state.value), _bits(b.timeseries_state.value)), f"{what}: particles differ"


def _same_rows(a, b):
    torch.testing.assert_close(a.filter_means, b.filter_means, rtol=1e-9, atol=1e-11)
    torch.testing.assert_close(a.filter_variance, b.filter_variance, rtol=1e-8, atol=1e-11)
    torch.testing.assert_close(a.loglikelihood, b.loglikelihood, rtol=1e-9, atol=1e-9)


def _one_piece_and_move_by_move(case, dtype=F64, **kwargs):
    y = _observations(case, dtype)
    out = []
    for moves in (False, True):
        filt = _filter(case, dtype, **kwargs)
        filt._move_by_move = moves
        out.append(filt.batch_filter(y, bar=False))
        torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("model,prop,n,b,tile_target,multi", [("sine", "lgo", 1 << 16, 1, 0, 0), ("sv_batched", "bootstrap", 8192, 8, 16, 1)],
                         ids=["single_round_65536x1", "multi_round_8x8192"])
def test_interior_log_weights_are_not_stored(model, prop, n, b, tile_target, multi, dtype, monkeypatch):
    """A one-piece APF run of an even number of observed steps, no state history.  The log-weight slot that does not hold the
    initial state is filled with NaN before the run: states 1, 3, ... land there and all of them are interior, so the sentinel
    survives in every element, while the final state (slot ``T & 1 = 0``) is complete - finite log-weights, sorted ancestors
    inside ``[0, N)``.  (There is ONE ancestor buffer: its interior stores cannot be seen this way - the WRITE_SIZE counter
    does, profiles/interior_stores_traffic.txt.)  The run is the plan's second, i.e. the replayed hipGraph ``bench.py`` times."""
    monkeypatch.setattr(HINTS, "tile_target", tile_target)  # (8 x 8192 in tiles of four rounds: the MULTI instantiations)
    t_len = 6
    case = _case(model, "apf", prop, n, b, t_len)
    y = _observations(case, dtype)
    assert not bool(y.isnan().any())
    filt = _filter(case, dtype)
    filt.batch_filter(y, bar=False)  # (allocates the plan, launches directly)
    plan = filt._last_run["plan"]
    assert plan.ring == 0
    sentinel = plan.logw[1]
    sentinel.fill_(float("nan"))
    res = filt.batch_filter(y, bar=False)
    torch.cuda.synchronize()
    assert filt._last_run["plan"] is plan and plan.graph is not None, "the second run should replay the plan's graph"
    trace = ops.debug_launch_trace(t_len)
    assert [r["step"] for r in trace] == list(range(t_len)) and all(r["MULTI"] == multi for r in trace), trace
    if dtype == F32:  # the steady-state instantiation at every interior step, the generic one at the end
        assert [r["SPEC"] for r in trace] == [1] * (t_len - 1) + [0], trace
    assert bool(sentinel.isnan().all()), f"{int((~sentinel.isnan()).sum())} interior log-weights were stored"
    assert bool(torch.isfinite(plan.logw[0]).all()), "the final state's log-weights are incomplete"
    anc = plan.anc.long()
    assert int(anc.min()) >= 0 and int(anc.max()) < n and bool((anc[:, 1:] >= anc[:, :-1]).all()), "the final ancestors are incomplete"
    last = res.latest_state
    assert bool(torch.isfinite(last.weights).all()) and bool(torch.isfinite(res.loglikelihood).all())
    assert torch.equal(ops.to_cols(last.previous_indices.to(torch.int32)), plan.anc)


@pytest.mark.parametrize("model,prop,n,b", [("sine", "lgo", 8192, 3), ("sv_batched", "bootstrap", 4096, 4)])
def test_an_unobserved_step_still_finds_the_carried_weights(model, prop, n, b):
    """Observed -> NaN -> observed rows inside one piece: the step before a NaN row stores its log-weights (the propagate-only
    step reads and carries them), the NaN step stores them too."""
    case = _case(model, "apf", prop, n, b, 9, nan_steps=(2, 5, 6))
    one, moves = _one_piece_and_move_by_move(case)
    _same_state(one.latest_state, moves.latest_state, "one piece vs move by move")
    _same_rows(one, moves)
    assert bool(torch.isfinite(one.loglikelihood).all())


def _reissue(plan, x0, lw0, anc0, pieces):
    """The run of ``plan`` again on its own buffers, draws and epoch, as ``pieces`` of ``(t0, n_steps, finalize, resume,
    prepare_next)``; returns the final state's planes."""
    a, lib = plan.args, L.load()
    plan.x[0].copy_(x0)
    plan.logw[0].copy_(lw0)
    plan.anc.copy_(anc0)
    plan.ll_total.zero_()
    steps = 0
    for t0, n_steps, fin, resume, prepare in pieces:
        a.hints.resume, a.hints.prepare_next = resume, prepare
        L.check(lib.pf_filter_run(C.byref(a), t0, n_steps, fin, L.stream_ptr()), "pf_filter_run")
        steps = t0 + n_steps
    a.hints.resume = a.hints.prepare_next = 0
    torch.cuda.synchronize()
    slot = steps & 1
    return dict(x=plan.x[slot].clone(), logw=plan.logw[slot].clone(), anc=plan.anc.clone(), means=plan.means.clone(),
                vars=plan.vars.clone(), ll=plan.ll_total.clone())


def _plan_of_a_first_run(case, dtype=F64):
    """A filter's first one-piece run (launched directly) with the planes of its initial state - what ``_reissue`` starts from."""
    y = _observations(case, dtype)
    filt = _filter(case, dtype)
    state = filt.initialize()
    x0 = ops.to_soa(state.timeseries_state.value, filt._batched, filt._has_event).clone()
    lw0 = ops.to_cols(state.weights).clone()
    anc0 = state.ancestors32().reshape(case["B"], case["N"]).clone()
    res = filt.batch_filter(y, bar=False, init_state=state)
    torch.cuda.synchronize()
    plan = filt._last_run["plan"]
    first = dict(x=plan.x[case["T"] & 1].clone(), logw=plan.logw[case["T"] & 1].clone(), anc=plan.anc.clone(), means=plan.means.clone(),
                 vars=plan.vars.clone(), ll=plan.ll_total.clone())
    return filt, plan, (x0, lw0, anc0), first, res


def _same_planes(a, b, what):
    for k in ("anc", "logw", "x"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"
    torch.testing.assert_close(a["means"], b["means"], rtol=1e-9, atol=1e-11)
    torch.testing.assert_close(a["vars"], b["vars"], rtol=1e-8, atol=1e-11)
    torch.testing.assert_close(a["ll"], b["ll"], rtol=1e-9, atol=1e-9)


def test_flags_derived_on_the_device_decide_in_the_kernel():
    """No ``observed`` array: the run derives the flags from ``y`` on the device and the kernels read them there (``obs = -1``) -
    whether the next step is observed, and with it whether this step's log-weights are dead, is decided in the kernel."""
    t_len = 9
    case = _case("sine", "apf", "lgo", 8192, 3, t_len, nan_steps=(2, 5, 6))
    filt, plan, init, first, _ = _plan_of_a_first_run(case)
    moves = _reissue(plan, *init, [(s, 1, 1, 0, 0) for s in range(t_len)])
    _same_planes(first, moves, "one piece (host flags) vs move by move")
    a = plan.args
    saved = a.observed
    a.observed, a.observed_dev = None, None
    try:
        derived = _reissue(plan, *init, [(0, t_len, 1, 0, 0)])
    finally:
        a.observed = saved
    _same_planes(derived, moves, "one piece (derived flags) vs move by move")
    for k in ("anc", "logw", "x", "means", "vars", "ll"):  # (the same launches as with host flags, but for where the flag is read)
        assert torch.equal(_bits(derived[k]), _bits(first[k])), k


def test_recorded_states_are_complete():
    """A state history (``ring >= 3``): every state is somebody's input (FilterResult.states, smoothing) - all stored."""
    case = _case("sine", "apf", "lgo", 8192, 3, 8)
    one, moves = _one_piece_and_move_by_move(case, record_states=True)
    assert len(one.states) == len(moves.states) == 9
    for q, (s1, s2) in enumerate(zip(one.states[1:], moves.states[1:]), start=1):
        _same_state(s1, s2, f"state {q}")
        assert bool(torch.isfinite(s1.weights).all())
    _same_rows(one, moves)


def test_a_prepared_piece_hands_its_whole_state_to_a_resumed_piece():
    """A piece that ends with ``prepare_next`` (no finalize) followed by a resumed piece that skips ``k_fused_reduce``: the first
    piece's last state keeps all its planes whatever the hints say, the second piece's interior states do not."""
    t_len = 8
    case = _case("sine", "apf", "lgo", 8192, 3, t_len)
    filt, plan, init, first, _ = _plan_of_a_first_run(case)
    moves = _reissue(plan, *init, [(s, 1, 1, 0, 0) for s in range(t_len)])
    _same_planes(first, moves, "one piece vs move by move")
    pieces = _reissue(plan, *init, [(0, 1, 0, 0, 1), (1, t_len - 1, 1, 1, 0)])
    _same_planes(pieces, moves, "prepared + resumed pieces vs move by move")
    chained = _reissue(plan, *init, [(s, 1, 1 if s == t_len - 1 else 0, 1 if s else 0, 0 if s == t_len - 1 else 1) for s in range(t_len)])
    _same_planes(chained, moves, "a chain of prepared / resumed moves vs move by move")


def test_sisr_keeps_its_ancestors_across_steps_that_do_not_resample():
    """SISR with a threshold that some steps cross and others do not: a step that does not resample leaves the ancestors of the
    last resampling step in place and carries the weights - SISR stores everything at every step."""
    case = _case("lg1d", "sisr", "bootstrap", 8192, 3, 12, ess=0.5)
    one, moves = _one_piece_and_move_by_move(case)
    _same_state(one.latest_state, moves.latest_state, "one piece vs move by move")
    _same_rows(one, moves)
    # the run really mixes both kinds of step: with a state history, a step that did not resample repeats its predecessor's ancestors
    y = _observations(case, F64)
    rec = _filter(case, F64, record_states=True).batch_filter(y, bar=False)
    kept = [torch.equal(s2.previous_indices, s1.previous_indices) for s1, s2 in zip(rec.states[1:-1], rec.states[2:])]
    assert any(kept) and not all(kept), kept
    _same_state(rec.latest_state, one.latest_state, "recorded vs plain run")
