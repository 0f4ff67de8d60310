"""The one-column leaf of the step kernel (``k_fused_step<..., ONECOL = true>``, ``pf_fused.hpp: OneColHeader``; the rule:
``pf_step.hip: filter_run_impl``) against the generic kernel it stands in for.

The leaf takes the APF steady state of ONE float column of 2^q >= 16 single-round tiles on the closed-form kernels when the launch
writes an interior state; every other launch - the run's last step, the steps around a NaN observation, a batch, a column whose
tile count is no power of two, multinomial resampling, float64 - takes the generic kernel.  It runs the same helpers in the same
order on the same operands, so its results are the generic kernel's BIT FOR BIT: every comparison here is ``torch.equal`` on bit
patterns, between two filter objects of the same seed that are issued the same sequence of calls (so their Philox epochs match) -
one on the library's own choice, one with ``_batch_filter(generic_steps=True)`` (``PF_ROUTE_PER_STEP_GENERIC``).

Shapes: 16 384 particles (16 tiles: the smallest column with an XCD tile map; the library's own choice there is the column-cluster
kernel, so the leaf's side is pinned to the per-step route) and 32 768 (32 tiles: reaches the leaf by default, through the general
driver - direct launch first, then a captured hipGraph)."""
import pytest
import torch

from oracle.cases import build_spec, simulate
from pyfilter_amd import ops
from tests.helpers import build_ssm_from_case

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
T_LEN = 16
NAN_AT = 7
# one-step predictive standard deviation of an observation (the optimal proposal's first-stage weights are taken under it):
# sqrt(a^2 g^2 dt + s^2) - sine diffusion: sigma = 1, dt = 0.1, s = 0.1 -> 0.33; OU (kappa 0.025, sigma 0.05, dt 1), s = 0.05 -> 0.07
PRED_STD = {"sine": 0.33, "ou_batched": 0.07}


def _case(model, prop, n, b=1, t_len=T_LEN, nan_steps=(NAN_AT,)):
    return dict(name=f"{model}_apf_{prop}", model=model, filter="apf", proposal=prop, N=n, B=b, T=t_len, ess_threshold=0.9, seed=4242,
                nan_steps=tuple(nan_steps))


def _filter(case, dtype, resampler="systematic"):
    from pyfilter_amd import resampling
    from pyfilter_amd.filters.particle import APF, proposals

    ssm = build_ssm_from_case(case, dtype, "cuda")
    prop = {"bootstrap": proposals.Bootstrap, "lgo": proposals.LinearGaussianObservations}[case["proposal"]]()
    rs = {"systematic": resampling.systematic, "multinomial": resampling.multinomial}[resampler]
    filt = APF(ssm, case["N"], proposal=prop, resampling=rs, ess_threshold=case["ess_threshold"], seed=31)
    if case["B"] > 1 or case["model"] == "ou_batched":  # (its parameters are rows of a batch, of one filter here)
        filt.set_batch_shape(torch.Size([case["B"]]))
    return filt


def _observations(case, dtype):
    return simulate(case, build_spec(case, F64)).to(dtype).cuda()


def _bits(t):
    """Bit pattern of a tensor (NaN-safe equality)."""
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def _planes(res):
    last = res.latest_state
    return dict(ll=res.loglikelihood, means=res.filter_means, variances=res.filter_variance, particles=last.timeseries_state.value,
                weights=last.weights, ancestors=last.previous_indices)


def _assert_same(a, b, what):
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"


def _run(filt, y, generic, per_step=False):
    """One ``batch_filter`` call of ``filt``: the library's own kernels (``per_step``: pinned to the per-step route) or the generic
    step kernels only; ``(planes, trace of the call's launches)``."""
    res = filt._batch_filter(y, per_step=per_step and not generic, generic_steps=generic)[0]
    torch.cuda.synchronize()
    return _planes(res), ops.debug_launch_trace(y.shape[0])


def _expected_spec(y):
    """SPEC of every launch of an APF run on ``y`` (float): 1 where this and the next observation carry information, else 0."""
    obs = [not bool(row.isnan().all()) for row in y]
    return [1 if (obs[t] and t + 1 < len(obs) and obs[t + 1]) else 0 for t in range(len(obs))]


def _assert_leaf_trace(trace, y, what):
    """The leaf ran on exactly the launches with SPEC = 1 that are not the run's last step - and they still report SPEC = 1, FAST = 1."""
    t_len = y.shape[0]
    assert [r["step"] for r in trace] == list(range(t_len)), (what, trace)
    assert [r["SPEC"] for r in trace] == _expected_spec(y), (what, trace)
    assert [r["LEAF"] for r in trace] == [1 if (r["SPEC"] == 1 and r["step"] != t_len - 1) else 0 for r in trace], (what, trace)
    assert sum(r["LEAF"] for r in trace) > 0 and all(r["FAST"] == 1 and r["MULTI"] == 0 for r in trace), (what, trace)


def _leaf_and_generic(case, y, dtype=F32, resampler="systematic", calls=1):
    """``calls`` consecutive runs of two filter objects of one seed, one on the library's own kernels and one on the generic step
    kernels only: ``[(planes, trace), ...]`` of either."""
    per_step = case["N"] <= 16384  # (the library's own choice there is the column-cluster kernel)
    own, gen = _filter(case, dtype, resampler), _filter(case, dtype, resampler)
    return ([_run(own, y, False, per_step) for _ in range(calls)], [_run(gen, y, True) for _ in range(calls)], own)


@pytest.mark.parametrize("n", [16384, 32768])
@pytest.mark.parametrize("model,prop", [("sine", "lgo"), ("ou_batched", "lgo"), ("sine", "bootstrap")],
                         ids=["sine_lgo_mk2", "ou_lgo_mk1", "sine_bootstrap_mk2"])
def test_leaf_equals_generic_bit_for_bit(model, prop, n):
    """16 steps with a NaN observation in the middle: the leaf hands over to generic launches (the step before the NaN row, the
    propagate-only step, the run's last step) and takes over again, so its partials and scans are checked as producer and as
    consumer.  ``sine_bootstrap``: the closed-form kernels take the proposal as an instantiation of their own - the leaf too."""
    case = _case(model, prop, n)
    y = _observations(case, F32)
    assert bool(y[NAN_AT].isnan()) and int(y.isnan().sum()) == 1
    own, gen, _ = _leaf_and_generic(case, y)
    _assert_leaf_trace(own[0][1], y, "leaf run")
    assert all(r["LEAF"] == 0 for r in gen[0][1]) and [r["SPEC"] for r in gen[0][1]] == _expected_spec(y), gen[0][1]
    assert own[0][1][0]["MK"] == gen[0][1][0]["MK"] == (2 if model == "sine" else 1)
    _assert_same(own[0][0], gen[0][0], f"{model} {prop} {n}")
    assert bool(torch.isfinite(own[0][0]["ll"]).all())


@pytest.mark.parametrize("n", [16384, 32768])
@pytest.mark.parametrize("model", ["sine", "ou_batched"])
def test_degenerate_weights(model, n):
    """One observation ~25 predictive standard deviations from the cloud: the weight sits on a few particles at the cloud's edge, so
    most tiles' windows start far from their ancestors - the window walk-on and the fallback search inside the leaf."""
    case = _case(model, "lgo", n)
    y = _observations(case, F32)
    y[4] = y[4] + 25.0 * PRED_STD[model]
    own, gen, _ = _leaf_and_generic(case, y)
    _assert_leaf_trace(own[0][1], y, "leaf run")
    _assert_same(own[0][0], gen[0][0], f"{model} outlier {n}")


def test_replay():
    """Three consecutive calls on each object - direct launch, graph capture, graph replay (the general driver at 32 768 particles):
    every call equals its twin.  The trace is written where a launch is ISSUED: the capture's records are the launches every
    later replay repeats, and they show the leaf; a replay issues none, so the records stay the capture's."""
    case = _case("sine", "lgo", 32768)
    y = _observations(case, F32)
    own, gen, filt = _leaf_and_generic(case, y, calls=3)
    plan = filt._last_run["plan"]
    assert plan.graph is not None and plan.runs == 3, "the second call should capture the plan's graph, the third replay it"
    for i, (a, b) in enumerate(zip(own, gen)):
        _assert_same(a[0], b[0], f"call {i}")
        _assert_leaf_trace(a[1], y, f"call {i}")
        assert all(r["LEAF"] == 0 for r in b[1])
    assert not torch.equal(_bits(own[0][0]["ll"]), _bits(own[1][0]["ll"])), "consecutive calls draw fresh numbers"


@pytest.mark.parametrize("model,n,b,resampler,dtype", [
    ("sine", 32768, 2, "systematic", F32),       # a batch
    ("sine", 32768 + 4, 1, "systematic", F32),   # 33 tiles, the last one of four particles
    ("sine", 3 * 16384, 1, "systematic", F32),   # 48 tiles: no power of two
    ("sine", 32768, 1, "multinomial", F32),
    ("sine", 32768, 1, "systematic", F64),
], ids=["batch_2x32768", "n_32772", "n_49152", "multinomial", "float64"])
def test_ineligible_shapes_stay_generic(model, n, b, resampler, dtype):
    case = _case(model, "lgo", n, b=b, t_len=8, nan_steps=())
    y = _observations(case, dtype)
    own, gen, _ = _leaf_and_generic(case, y, dtype=dtype, resampler=resampler)
    assert [r["step"] for r in own[0][1]] == list(range(8)) and all(r["LEAF"] == 0 for r in own[0][1]), own[0][1]
    _assert_same(own[0][0], gen[0][0], f"{n} x {b} {resampler}")
