"""NestedProposal on the GPU: the kernel (``csrc/pf_nested.hpp``) and the torch route against the unmodified reference's
fixtures (``tools/make_golden_nested.py``) and against the float64 oracle (``tests/nested_oracle.py``).

Float32 bar of the weights (tests 2 and 3), ``max |dw| / (1 + |w|)`` against the float64 oracle on the same rounded inputs.
The package's own torch route in float32 was measured on the MI355X on exactly these inputs (every weighted step of the float32
fixtures plus one synthetic call of >= 20 000 particles per model; ``tools/nested_f32_bar.py cuda``, ``profiles/nested_proposal.txt``;
the same tool on a CPU gives 1.7e-7 / 7.9e-7 / 3.6e-7 / 3.9e-6):

    stochastic volatility  1.7e-7      sine diffusion  8.6e-7      2-D random walk  3.5e-7      Lorenz-63  3.9e-6

The kernel's own worst figures on them: 2.4e-7 / 8.2e-7 / 4.2e-7 / 3.0e-6, no pick differing.

(Lorenz: |x| ~ 25 observed with s = 0.32 - a float32 ulp of the state is 2e-6, its residual is squared over 2 s^2 = 0.2.)  The kernel
is allowed 4x its model's figure.  Picks may differ from the oracle's for at most 1e-4 of the particles."""
import ctypes as C
import math

import pytest
import torch

from oracle import cpu_ref
from pyfilter_amd import _lib as L
from pyfilter_amd import ops
from pyfilter_amd.hints import HINTS
from tests import nested_cases as nc
from tests.helpers import build_ssm_from_case, load_golden
from tests.nested_oracle import assert_weights_match
from tools.make_golden_nested import CASES

pytestmark = pytest.mark.gpu

TORCH_F32_ERR = {"sv_batched": 1.7e-7, "sine": 8.6e-7, "rw2d": 3.5e-7, "lorenz": 3.9e-6}  # measured (module docstring)
F32_BAR = {k: 4.0 * v for k, v in TORCH_F32_ERR.items()}
PICK_BAR = 1e-4
F64_CASES = [c for c in CASES if "f64" in c["dtypes"]]


_context, run_kernel = nc.kernel_context, nc.run_kernel


def check_call(call):
    """Kernel against oracle: float64 1e-12 relative, float32 the model's bar; picks within PICK_BAR, kept candidates equal where
    the picks agree (float32: the suite's float32 tolerance of recorded states, rtol 2e-5 / atol 2e-6)."""
    x, w, pick = run_kernel(call)
    err, miss = nc.weight_error(w, call.ref_w), nc.pick_mismatch(pick, call.ref_pick)
    print(f"{call.name} {call.dtype}: weight error {err:.3e}, picks differing {miss:.2e}")
    assert bool(((pick >= 0) & (pick < call.m)).all())
    same = pick == call.ref_pick
    if call.dtype == torch.float64:
        assert err <= 1e-12 and miss == 0.0
        torch.testing.assert_close(x.double()[same], call.ref_x[same], rtol=1e-12, atol=1e-12)
    else:
        assert err <= F32_BAR[call.case["model"]] and miss <= PICK_BAR
        torch.testing.assert_close(x.double()[same], call.ref_x[same], rtol=2e-5, atol=2e-6)
    return x, w, pick


# --------------------------------------------------------------------------------------------------- 1. end to end, float64
def _run_filter(case, g, dtype, kernel: bool, monkeypatch):
    from pyfilter_amd.filters.particle import APF, SISR, proposals

    monkeypatch.setattr(HINTS, "nested_kernel", kernel)
    ssm = build_ssm_from_case(case, dtype, "cuda")
    prop = proposals.NestedProposal(case["M"])
    prop.record_picks = True
    prop.set_tape(z=g["z_tape"].to(dtype), v=g["v_tape"].to(dtype))
    filt = {"sisr": SISR, "apf": APF}[case["filter"]](ssm, case["N"], proposal=prop, ess_threshold=case["ess_threshold"])
    filt.set_batch_shape(torch.Size([case["B"]]))
    filt.set_tape(u=g["u_tape"].to(dtype), z0=g["z0"].to(dtype))
    state = filt.initialize()
    assert prop.uses_kernels == kernel
    torch.testing.assert_close(state.timeseries_state.value.cpu(), g["x0"].to(dtype), rtol=1e-12, atol=1e-12)
    result = filt.initialize_with_result(state)
    out = {k: [] for k in ("x", "w", "ll", "idx", "pick")}
    y = g["y"].to(dtype).cuda()
    for t in range(case["T"]):
        prop.last_pick = None
        state = filt.filter(y[t], state, result=result)
        out["x"].append(state.timeseries_state.value.cpu())
        out["w"].append(state.weights.cpu().clone())
        out["ll"].append(state.get_loglikelihood().cpu().clone())
        out["idx"].append(state.previous_indices.cpu().clone())
        out["pick"].append(prop.last_pick.cpu() if prop.last_pick is not None else torch.full((case["N"], case["B"]), -1))
    res = {f"step_{k}": torch.stack(v) for k, v in out.items()}
    res["filter_means"], res["loglikelihood"] = result.filter_means.cpu(), result.loglikelihood.cpu()
    return res


@pytest.mark.parametrize("route", ["kernel", "torch"])
@pytest.mark.parametrize("case", F64_CASES, ids=lambda c: c["name"])
def test_filter_matches_reference_f64(case, route, monkeypatch):
    g = load_golden(case["name"], "f64")
    out = _run_filter(case, g, torch.float64, route == "kernel", monkeypatch)
    assert torch.equal(out["step_idx"], g["step_idx"].long()), "ancestors differ from the reference"
    assert torch.equal(out["step_pick"], g["step_pick"].long()), "picks differ from the reference"
    tol = dict(rtol=1e-9, atol=1e-9)
    for k in ("step_x", "step_ll", "filter_means", "loglikelihood"):
        torch.testing.assert_close(out[k], g[k], equal_nan=True, **tol)
    assert_weights_match(out["step_w"], g["step_w"], **tol)  # (the shifted weight where the reference's underflowed: INTEGRATION.md)


# --------------------------------------------------------------------------------- 2. float32 kernels, teacher-forced per step
@pytest.fixture(scope="module")
def f32_calls():
    return nc.f32_inputs()


def test_f32_kernel_against_f64_oracle(f32_calls):
    assert sum(c.n * c.b >= 20000 for c in f32_calls) == 4
    worst = {}
    for call in f32_calls:
        _, w, pick = check_call(call)
        k = call.case["model"]
        worst[k] = max(worst.get(k, 0.0), nc.weight_error(w, call.ref_w))
    print("worst float32 weight error per model:", {k: f"{v:.2e}" for k, v in worst.items()}, "bars:", F32_BAR)


# ------------------------------------------------------------------------------------------- 3. shapes where it can go wrong
BOTH = [torch.float64, torch.float32]


@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
@pytest.mark.parametrize("model,n,b", [("sv_batched", 300, 3), ("sine", 257, 2), ("lorenz", 130, 2), ("rw2d", 300, 3)])
def test_one_candidate_is_bootstrap_bit_for_bit(model, n, b, dtype):
    call = nc.synthetic(model, n, b, 1, dtype, seed=1, negative_third=(model == "sv_batched"))
    x, w, pick = run_kernel(call)
    kind, params, has_event = _context(call.case, b, n, 1, dtype)
    z_soa = ops.to_soa(call.z[0].cuda(), True, has_event)
    xb, wb = ops.sample_and_weight_soa(kind, params, L.PROP_BOOTSTRAP, ops.to_soa(call.x.cuda(), True, has_event), call.y.cuda(), z_soa, 7, 3)
    xb, wb = ops.from_soa(xb, True, has_event).cpu(), wb.t().cpu()
    assert torch.equal(x, xb) and bool((pick == 0).all())
    finite = wb.isfinite()
    assert bool(finite.any()) and torch.equal(w[finite], wb[finite])
    assert bool((w[~finite] == -math.inf).all())  # (Bootstrap's NaN / +inf - sanitised later by normalize - is -inf here)


@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
@pytest.mark.parametrize("model,n,b,m,kw", [
    ("sv_batched", 300, 3, 5, {}),                      # ragged last block, per-filter parameter rows, y_rows = B
    ("sv_batched", 300, 3, 5, dict(shared_y=True)),     # ... y_rows = 1
    ("sv_batched", 1, 1, 64, {}),                       # N = 1
    ("sine", 300, 2, 64, {}),
    ("sine", 1, 2, 5, {}),
    ("lorenz", 300, 2, 5, {}),                          # D = 3, O = 2
    ("rw2d", 300, 3, 64, {}),                           # D = 2, O = 2
    ("rw2d", 513, 1, 256, {}),                          # PF_NESTED_MAX candidates
])
def test_kernel_shapes(model, n, b, m, kw, dtype):
    check_call(nc.synthetic(model, n, b, m, dtype, seed=2, **kw))


def test_grid_stride_second_trip():
    """N = 2048 * PF_BLOCK + 77: the grid is capped at 2048 blocks, so the last 77 particles are a block's second trip."""
    call = nc.synthetic("sv_batched", 2048 * 256 + 77, 1, 2, torch.float32, seed=3)
    x, w, pick = check_call(call)
    tail = slice(2048 * 256, None)
    assert nc.pick_mismatch(pick[tail], call.ref_pick[tail]) == 0.0 and bool(w[tail].isfinite().all())


@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_all_candidates_invalid(dtype):
    m = 5
    call = nc.synthetic("sv_batched", 999, 2, m, dtype, seed=4, negative_third=True)
    x, w, pick = check_call(call)
    bad = (call.x < 0).cpu()
    assert bool(bad[::3].all()) and int(bad.sum()) >= 999 * 2 // 3
    assert bool((w[bad] == -math.inf).all()) and bool(w[~bad].isfinite().all())
    expect = (call.v.double() * m).floor().long().clamp(max=m - 1)
    assert torch.equal(pick[bad], expect[bad])


def _raw_call(model_struct, m, n, b, dtype):
    x = torch.ones((model_struct.dim, b, n), dtype=dtype, device="cuda")
    y = torch.zeros((1, model_struct.obs_dim), dtype=dtype, device="cuda")
    xo, wo = torch.empty_like(x), torch.empty((b, n), dtype=dtype, device="cuda")
    rc = L.load().pf_nested_sample_and_weight(C.byref(model_struct), m, x.data_ptr(), y.data_ptr(), 1, None, None, 1, 0, xo.data_ptr(),
                                              wo.data_ptr(), None, n, b, L.dtype_code(dtype), L.stream_ptr())
    torch.cuda.synchronize()
    return rc


def test_argument_checks():
    kind, params, _ = _context(nc.MODEL_CASE["sine"], 1, 64, 4, torch.float32)
    ms = ops.make_model_struct(kind, params)
    einval, eunsupported = -1, -3  # include/pf_amd.h: PF_EINVAL, PF_EUNSUPPORTED
    assert _raw_call(ms, 256, 64, 1, torch.float32) == 0
    assert _raw_call(ms, 257, 64, 1, torch.float32) == einval
    assert _raw_call(ms, 0, 64, 1, torch.float32) == einval
    assert _raw_call(ms, -3, 64, 1, torch.float32) == einval
    ms.hid_kind, ms.dim, ms.obs_dim = L.HID_LINEAR_MAT, 2, 2
    assert _raw_call(ms, 4, 64, 1, torch.float32) == eunsupported


@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_a_call_is_a_function_of_seed_and_step(dtype):
    call = nc.synthetic("sv_batched", 700, 2, 7, dtype, seed=5)
    a, b2 = run_kernel(call, z=False, seed=11, step=4), run_kernel(call, z=False, seed=11, step=4)
    other_step, other_seed = run_kernel(call, z=False, seed=11, step=5), run_kernel(call, z=False, seed=12, step=4)
    assert all(torch.equal(p, q) for p, q in zip(a, b2))
    assert not torch.equal(a[0], other_step[0]) and not torch.equal(a[0], other_seed[0])
    assert bool(a[1].isfinite().all()) and len(a[2].unique()) == 7  # every candidate index is taken by somebody


# ------------------------------------------------------------------------------------------------------------ 4. statistics
def test_ar1_against_the_kalman_filter_on_philox_draws():
    """SISR, AR(1) (beta 0.9, sigma 0.5, s 0.2, x0 ~ N(0, 0.5)), T = 20, N = 256, B = 64 filters, M = 16, float32, the kernels' own
    draws.  (i) mean over filters of exp(ll - ll_Kalman) is 1 within 4 standard errors (the estimate is unbiased); (ii) the
    filter-averaged filter means on the Kalman means: max |z| <= 12, mean z^2 <= 3 (tests/test_linear_model_gpu.py's bound);
    (iii) sd of ll over the filters <= 0.6 x Bootstrap's at the same N on the same data (the reference: 0.30 - 0.38) - a pick
    that ignored the weights or a weight that was not the mean would fail it."""
    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.filters.particle import SISR, proposals
    from pyfilter_amd.timeseries import models

    beta, sigma, s, t_len, n, b = 0.9, 0.5, 0.2, 20, 256, 64
    gen = torch.Generator().manual_seed(21)
    x, ys = 0.5 * torch.randn((), generator=gen, dtype=torch.float64), []
    for _ in range(t_len):
        x = beta * x + sigma * torch.randn((), generator=gen, dtype=torch.float64)
        ys.append(x + s * torch.randn((), generator=gen, dtype=torch.float64))
    y = torch.stack(ys)
    km, kll = cpu_ref.kalman_filter_1d(y, 0.0, beta, sigma, 1.0, 0.0, s, 0.0, 0.25)
    t = lambda v: torch.tensor(v, dtype=torch.float32, device="cuda")  # noqa: E731

    def run(prop):
        ssm = ts.LinearStateSpaceModel(models.AR(t(0.0), t(beta), t(sigma), initial=(t(0.0), t(0.5))), (t(1.0), t(s)))
        filt = SISR(ssm, n, proposal=prop, seed=5)
        filt.set_batch_shape(torch.Size([b]))
        res = filt.batch_filter(y.float().cuda(), bar=False)
        return res.loglikelihood.double().cpu(), res.filter_means[1:, :, 0].double().cpu()

    ll, means = run(proposals.NestedProposal(16))
    ll_boot, _ = run(proposals.Bootstrap())
    ratio = (ll - kll).exp()
    z_ll = float((ratio.mean() - 1.0) / (ratio.std() / math.sqrt(b)))
    zs = (means.mean(1) - km) / (means.std(1) / math.sqrt(b) + 1e-12)
    print(f"z(exp(ll - kalman)) = {z_ll:.2f}, max |z| of means {float(zs.abs().max()):.2f}, mean z^2 {float(zs.square().mean()):.2f}, "
          f"sd(ll) nested {float(ll.std()):.3f} bootstrap {float(ll_boot.std()):.3f}")
    assert abs(z_ll) <= 4.0
    assert float(zs.abs().max()) <= 12.0 and float(zs.square().mean()) <= 3.0
    assert float(ll.std()) <= 0.6 * float(ll_boot.std())


# ------------------------------------------------------------------------------------------------------------ 5. user lambda
def test_user_lambda_takes_the_torch_route_and_agrees():
    from torch.distributions import Normal

    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.filters.particle import SISR, proposals
    from pyfilter_amd.timeseries import models

    t = lambda v: torch.tensor(v, device="cuda")  # noqa: E731
    gen = torch.Generator().manual_seed(31)
    x, ys = torch.randn((), generator=gen), []
    for _ in range(10):
        x = x + torch.sin(x) * 0.1 + math.sqrt(0.1) * torch.randn((), generator=gen)
        ys.append(x + 0.1 * torch.randn((), generator=gen))
    y = torch.stack(ys).cuda()
    sine = ts.AffineEulerMaruyama(lambda x, gamma, sigma: (torch.sin(x.value - gamma), sigma), (t(0.0), t(1.0)),
                                  Normal(t(0.0), t(math.sqrt(0.1))), dt=0.1, initial_kernel=lambda g, s: Normal(t(0.0), t(1.0)))
    lls = []
    for hidden, kernels in ((sine, False), (models.SineDiffusion(t(0.0), t(1.0), dt=0.1), True)):
        prop = proposals.NestedProposal(8)
        filt = SISR(ts.LinearStateSpaceModel(hidden, (t(1.0), t(0.1))), 512, proposal=prop, seed=9)
        filt.set_batch_shape(torch.Size([32]))
        lls.append(filt.batch_filter(y, bar=False).loglikelihood.double().cpu())
        assert prop.uses_kernels == kernels
    se = math.sqrt(float(lls[0].var()) / 32 + float(lls[1].var()) / 32)
    print(f"mean ll: lambda {float(lls[0].mean()):.4f}, built-in {float(lls[1].mean()):.4f}, se {se:.4f}")
    assert bool(lls[0].isfinite().all()) and abs(float(lls[0].mean() - lls[1].mean())) <= 6.0 * se


# ----------------------------------------------------------------------------------------------------------------- 6. SMC^2
def test_smc2_runs_with_the_nested_proposal():
    from torch.distributions import Exponential, LogNormal

    from pyfilter_amd.filters.particle import APF, proposals
    from pyfilter_amd.inference import SMC2
    from pyfilter_amd.timeseries import models

    gen = torch.Generator().manual_seed(41)
    v, ys = torch.tensor(1.0), []
    for _ in range(31):
        v = v + 0.05 * (1.0 - v) * v * 0.2 + 0.1 * v * math.sqrt(0.2) * torch.randn((), generator=gen)
        ys.append(v * torch.randn((), generator=gen))
    y = torch.stack(ys).cuda()
    t = lambda val: torch.tensor(val, device="cuda")  # noqa: E731

    def build_sv(theta):
        return models.StochasticVolatilityModel(models.Verhulst(theta["kappa"], theta["gamma"], theta["sigma"], dt=0.2,
                                                                initial=(t(1.0), t(0.1))), t(0.0))

    priors = {"kappa": Exponential(10.0), "gamma": LogNormal(0.0, 0.2), "sigma": LogNormal(-2.0, 0.5)}
    alg = SMC2(APF(build_sv, 128, proposal=proposals.NestedProposal(4)), 64, priors, threshold=0.5, device="cuda", seed=2)
    state = alg.fit(y[:30])
    assert bool(alg.posterior_mean(state).isfinite().all())
    state = alg.step(y[30], state)
    assert state.current_iteration == 31 and bool(state.w.isfinite().all()) and bool(alg.posterior_mean(state).isfinite().all())


# ------------------------------------------------------------------------------- 7. the routes' shared edge cases and limits
@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_running_sum_that_never_passes_keeps_the_last_live_candidate(dtype):
    """``v = 1`` and an invalid last candidate (tests/nested_cases.py): the kernel, like the torch route and the oracle, keeps the last
    candidate of positive weight."""
    call = nc.last_candidate_invalid(dtype)
    x, w, pick = run_kernel(call)
    assert bool((pick == call.m - 2).all()) and bool((call.ref_pick == call.m - 2).all()) and bool(w.isfinite().all())
    _, w_t, pick_t = nc.torch_route(call, "cuda")
    assert bool((pick_t.cpu() == call.m - 2).all())


@pytest.mark.parametrize("name", ["nested_lorenz_sisr", "nested_sv_apf"])
def test_torch_route_in_slices_matches_reference_f64(name, monkeypatch):
    """The torch route with its slices forced small (37 particles per slice or fewer): still the reference's run."""
    from pyfilter_amd.filters.particle.proposals import NestedProposal

    case = next(c for c in CASES if c["name"] == name)
    monkeypatch.setattr(NestedProposal, "TORCH_CANDIDATES", 37 * case["M"] * (3 if "lorenz" in name else 1))
    g = load_golden(name, "f64")
    out = _run_filter(case, g, torch.float64, False, monkeypatch)
    assert torch.equal(out["step_idx"], g["step_idx"].long()) and torch.equal(out["step_pick"], g["step_pick"].long())
    tol = dict(rtol=1e-9, atol=1e-9)
    for k in ("step_x", "step_ll", "filter_means", "loglikelihood"):
        torch.testing.assert_close(out[k], g[k], equal_nan=True, **tol)
    assert_weights_match(out["step_w"], g["step_w"], **tol)
