"""Linear-Gaussian models of 4 to 8 state components on the GPU: the stand-alone primitives at any state dimension, the
``PF_HID_LINEAR_MAT`` model kernels against the reference's fixtures (``tools/make_golden_linear.py``; tape mode), the same
models on the torch route, exactness against the Kalman filter on the kernels' own draws, and theta on the batch dimension."""
import math

import pytest
import torch

from oracle import cpu_ref
from tests import linear_cases as LC

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- primitives
@pytest.mark.parametrize("d", [4, 5, 8, 13])
@pytest.mark.parametrize("n", [1000, 70000])  # one tile / several tiles per column
def test_primitives_at_large_state_dimension(d, n):
    from pyfilter_amd import ops

    g = torch.Generator(device="cuda").manual_seed(d * 1000 + n)
    b = 3
    x = (torch.randn((d, b, n), generator=g, device="cuda", dtype=torch.float64) * 2.0 + 0.5).contiguous()
    W = torch.softmax(torch.randn((b, n), generator=g, device="cuda", dtype=torch.float64), 1).contiguous()
    mean, var = ops.moments_soa(x, W)
    m_ref = torch.einsum("dbn,bn->bd", x, W)
    v_ref = torch.einsum("dbn,bn->bd", (x - m_ref.t().unsqueeze(-1)) ** 2, W)
    torch.testing.assert_close(mean, m_ref, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(var, v_ref, rtol=1e-12, atol=1e-14)

    for dtype in (torch.float32, torch.float64):
        z = torch.randn((d, b, n), generator=g, device="cuda", dtype=torch.float64).to(dtype)
        m0 = [0.1 * k for k in range(d)]
        s0 = [1.0 + 0.5 * k for k in range(d)]
        xs = ops.initial_sample_soa(m0, s0, n, b, d, dtype, torch.device("cuda"), seed=5, z=z)
        mt = torch.tensor(m0, dtype=dtype, device="cuda").view(d, 1, 1)
        st = torch.tensor(s0, dtype=dtype, device="cuda").view(d, 1, 1)
        # (pf_initial_sample forms m + s z as one fused multiply-add, as it always has for D <= 3: within one rounding of the
        # larger term; the per-filter kernel below keeps the two roundings of torch's expression - bit-exact)
        eps = torch.finfo(dtype).eps
        assert ((xs - (mt + st * z)).abs() <= eps * (mt.abs() + (st * z).abs())).all()
        mc = torch.randn((b, d), generator=g, device="cuda", dtype=torch.float64).to(dtype)
        sc = torch.rand((b, d), generator=g, device="cuda", dtype=torch.float64).to(dtype) + 0.1
        xc = ops.initial_sample_cols(mc, sc, n, b, d, seed=5, z=z)
        assert torch.equal(xc, mc.t().unsqueeze(-1) + sc.t().unsqueeze(-1) * z)
        # Philox draws: every plane its own standard normals
        xp = ops.initial_sample_soa([0.0] * d, [1.0] * d, n, b, d, dtype, torch.device("cuda"), seed=5)
        assert xp.double().mean().abs() < 0.05 and (xp.double().std() - 1.0).abs() < 0.05
        assert not torch.equal(xp[0], xp[3 % d]) or d < 4

    s = 6
    xh = torch.randn((s, d, b, n), generator=g, device="cuda", dtype=torch.float64)
    anc = torch.randint(0, n, (s, b, n), generator=g, device="cuda", dtype=torch.int32)
    out = ops.smooth_fixed_lag(xh, anc)
    idx = torch.arange(n, device="cuda").expand(b, n)
    for t in range(s - 1, -1, -1):
        assert torch.equal(out[t], xh[t].gather(2, idx.unsqueeze(0).expand(d, b, n)))
        idx = anc[t].long().gather(1, idx)


# ---------------------------------------------------------------------------------------------- reference parity (kernels)
@pytest.mark.parametrize("name,dt", LC.PARAMS)
def test_model_kernels_teacher_forced_against_the_reference(name, dt):
    """Move by move from the reference's own state t (resampled with its recorded ancestors): ``pf_sample_and_weight`` /
    ``pf_pre_weight`` of ``PF_HID_LINEAR_MAT`` with the recorded normals give the reference's particles and weights - float64 to
    1e-9, float32 to the bars of the existing float32 suites (particles 2e-4 relative / 2e-5 absolute, log-weights 1e-4 relative
    / 2e-3 absolute)."""
    from pyfilter_amd import _lib as L
    from pyfilter_amd import ops

    g = LC.load(name, dt)
    dtype = LC.DT[dt]
    filt_name, prop_name, ess, _ = LC.CASES[name]
    filt = LC.build_filter(name, g, dtype, "cuda")
    ctx = filt._ensure_context()
    kind, params = ctx.kind, ctx.params
    assert kind.hid_kind == L.HID_LINEAR_MAT
    code = L.PROP_LGO if prop_name == "lgo" else L.PROP_BOOTSTRAP
    tx = dict(rtol=1e-9, atol=1e-11) if dt == "f64" else dict(rtol=2e-4, atol=2e-5)
    tw = dict(rtol=1e-9, atol=1e-9) if dt == "f64" else dict(rtol=1e-4, atol=2e-3)
    n, b = g["x0"].shape[:2]
    x, w = g["x0"].to(dtype), torch.zeros(n, b, dtype=dtype)
    for t in range(g["y"].shape[0]):
        y, idx = g["y"][t].to(dtype), g["step_idx"][t]
        if filt_name == "sisr":
            W = torch.softmax(w.double(), 0)
            mask = 1.0 / W.square().sum(0) < ess * n
            xr = torch.where(mask.view(1, b, 1), x.gather(0, idx.unsqueeze(-1).expand_as(x)), x)
            wr = torch.where(mask.view(1, b), torch.zeros_like(w), w)
        else:
            xr = x.gather(0, idx.unsqueeze(-1).expand_as(x))
        soa = ops.to_soa(xr.cuda(), True, True).contiguous()
        z = ops.to_soa(g["z_tape"][t].to(dtype).cuda(), True, True).contiguous()
        observed = not torch.isnan(y).all()
        x_out, w_out = ops.sample_and_weight_soa(kind, params, code, soa, y.cuda() if observed else None, z, 0, t, weigh=observed)
        torch.testing.assert_close(ops.from_soa(x_out, True, True).cpu(), g["step_x"][t], **tx)
        if not observed:
            w_new = wr
        elif filt_name == "sisr":
            w_new = ops.from_cols(w_out, True).cpu() + wr
        else:
            pre = ops.from_cols(ops.pre_weight_soa(kind, params, code, ops.to_soa(x.cuda(), True, True).contiguous(), y.cuda()), True).cpu()
            w_new = ops.from_cols(w_out, True).cpu() - pre.gather(0, idx)
        torch.testing.assert_close(w_new, g["step_w"][t], **tw)
        x, w = g["step_x"][t], g["step_w"][t]


@pytest.mark.parametrize("name,dt", [p for p in LC.PARAMS if p[1] == "f64"])
def test_model_kernels_match_the_reference(name, dt):
    """float64, tape mode: the filter as a whole - every move, the moments and the log-likelihood - on the reference's numbers."""
    from pyfilter_amd import _lib as L

    g = LC.load(name, dt)
    dtype = LC.DT[dt]
    filt = LC.build_filter(name, g, dtype, "cuda")
    assert filt._model.kernel_kind.hid_kind == L.HID_LINEAR_MAT and not filt._fused_capable(torch.device("cuda"))
    y = g["y"].to(device="cuda", dtype=dtype)
    state = LC.start_at_x0(filt, g, "cuda")
    assert filt._proposal.uses_kernels
    result = filt.initialize_with_result(state)
    tol = dict(rtol=1e-9, atol=1e-11)
    for t in range(y.shape[0]):
        state = filt.filter(y[t], state, result=result)
        torch.testing.assert_close(state.timeseries_state.value.cpu(), g["step_x"][t], **tol)
        torch.testing.assert_close(state.weights.cpu(), g["step_w"][t], equal_nan=True, **tol)
        torch.testing.assert_close(state.get_loglikelihood().cpu(), g["step_ll"][t], rtol=1e-9, atol=1e-9)
        assert torch.equal(state.previous_indices.cpu(), g["step_idx"][t]), f"ancestors differ at move {t}"
    torch.testing.assert_close(result.filter_means.cpu(), g["filter_means"], rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(result.loglikelihood.cpu(), g["loglikelihood"], rtol=1e-9, atol=1e-9)
    res = filt.batch_filter(y, bar=False, init_state=LC.start_at_x0(filt, g, "cuda"))  # (the whole run on the same tapes)
    torch.testing.assert_close(res.loglikelihood.cpu(), g["loglikelihood"], rtol=1e-9, atol=1e-9)


def test_fixed_lag_and_ffbs_smoothing_of_the_matrix_kind():
    name = "cv4d_apf_lgo"
    g = LC.load(name, "f64")
    filt = LC.build_filter(name, g, torch.float64, "cuda")
    state = LC.start_at_x0(filt, g, "cuda")
    states = [state]
    for t in range(g["y"].shape[0]):
        state = filt.filter(g["y"][t].cuda(), state)
        states.append(state)
    fl = filt.smooth(states, "fl")
    torch.testing.assert_close(fl.cpu(), g["smooth_fl"], rtol=1e-9, atol=1e-11)
    # ffbs: the torch-logits route user processes take, run on the kernels' states - and the same draws through a torch-route
    # copy of the model (the lambda) give the same trajectories
    torch.manual_seed(11)
    ff = filt.smooth(states, "ffbs")
    assert ff.shape == fl.shape and torch.isfinite(ff).all()
    lam = LC.build_filter(name, g, torch.float64, "cuda", how="lambda")
    lam._ensure_context()
    torch.manual_seed(11)
    ff2 = lam.smooth(states, "ffbs")
    torch.testing.assert_close(ff, ff2, rtol=1e-12, atol=1e-12)


# --------------------------------------------------------------------------------------------------------- torch route
@pytest.mark.parametrize("name", list(LC.CASES))
def test_the_same_model_as_a_user_lambda_runs_end_to_end(name):
    """The model written as a plain AffineProcess lambda has no kernel kind at these dimensions: torch model arithmetic with the
    HIP primitives underneath (moments, resampling, gathers).  The whole run, then both smoothers."""
    g = LC.load(name, "f64")
    filt = LC.build_filter(name, g, torch.float64, "cuda", how="lambda", tape=False, record_states=True)
    assert filt._model.kernel_kind is None
    res = filt.batch_filter(g["y"].cuda(), bar=False)
    t_len, (n, b, d) = g["y"].shape[0], g["x0"].shape
    assert res.filter_means.shape == (t_len + 1, b, d) and torch.isfinite(res.filter_means).all()
    assert torch.isfinite(res.loglikelihood).all()
    states = res.states
    assert len(states) == t_len + 1
    fl = filt.smooth(states, "fl")
    ff = filt.smooth(states, "ffbs")
    assert fl.shape == ff.shape == (t_len + 1, n, b, d) and torch.isfinite(fl).all() and torch.isfinite(ff).all()


# ---------------------------------------------------------------------------------------------- exactness on own draws
def _kalman_case(which):
    g = torch.Generator().manual_seed(77)
    if which == "cv4d":
        p = {k: v for k, v in LC.load("cv4d_sisr_boot", "f64").items()}
        A, b, s, Ao, bo, so, m0, s0 = (p[k].double() for k in ("hid_A", "hid_b", "hid_s", "obs_A", "obs_b", "obs_s", "init_m", "init_s"))
    else:
        d = o = 8
        A = 0.6 * torch.eye(d, dtype=torch.float64) + 0.25 * torch.randn(d, d, generator=g, dtype=torch.float64) / d ** 0.5
        b = 0.1 * torch.randn(d, generator=g, dtype=torch.float64)
        s = 0.1 + 0.1 * torch.rand(d, generator=g, dtype=torch.float64)
        Ao = torch.eye(d, dtype=torch.float64) + 0.5 * torch.randn(o, d, generator=g, dtype=torch.float64)
        bo = 0.1 * torch.randn(o, generator=g, dtype=torch.float64)
        so = 0.2 + 0.2 * torch.rand(o, generator=g, dtype=torch.float64)
        m0, s0 = torch.zeros(d, dtype=torch.float64), 0.5 * torch.ones(d, dtype=torch.float64)
    x, ys = m0 + s0 * torch.randn(len(m0), generator=g, dtype=torch.float64), []
    for _ in range(100):
        x = b + A @ x + s * torch.randn(len(b), generator=g, dtype=torch.float64)
        ys.append(bo + Ao @ x + so * torch.randn(len(bo), generator=g, dtype=torch.float64))
    return (A, b, s, Ao, bo, so, m0, s0), torch.stack(ys)


@pytest.mark.parametrize("which", ["cv4d", "lm8d"])
@pytest.mark.parametrize("prop", ["lgo", "bootstrap"])
def test_exact_against_the_kalman_filter_on_philox_draws(which, prop):
    """N = 65 536, T = 100, 8 seeds on the kernels' own Philox draws, standard errors taken over the 8 seeds.  Bars (stated):
    (i) the seeds' mean log-likelihood within 4 standard errors of the Kalman value; (ii) the seed-averaged filter means against
    the Kalman filtered means, z = (mean - kalman) / se per step and component: max |z| <= 12 and mean z^2 <= 3.  Under a correct
    filter z follows a Student t with 7 degrees of freedom (E z^2 = 1.4); with 400 - 800 comparisons per case a per-comparison
    bar of 4 is crossed a few times by chance (P(|t_7| > 4) = 0.5 %), 12 only with probability ~5e-3 per case (Bonferroni)."""
    from torch.distributions import Independent, Normal

    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.filters.particle import SISR, proposals
    from pyfilter_amd.timeseries import LinearModel

    (A, b, s, Ao, bo, so, m0, s0), y = _kalman_case(which)
    d, o = len(b), len(bo)
    km, kll = cpu_ref.kalman_filter(y.numpy(), A.numpy(), torch.diag(s * s).numpy(), Ao.numpy(), torch.diag(so * so).numpy(),
                                    m0.numpy(), torch.diag(s0 * s0).numpy(), c=b.numpy(), d=bo.numpy())
    cu = lambda t: t.cuda()  # noqa: E731
    lls, means = [], []
    for seed in range(8):
        inc = Independent(Normal(torch.tensor(0.0, dtype=torch.float64, device="cuda"), torch.tensor(1.0, dtype=torch.float64, device="cuda"))
                          .expand(torch.Size([d])), 1)
        hidden = LinearModel((cu(A), cu(b), cu(s)), inc, lambda *_: Independent(Normal(cu(m0), cu(s0)), 1))
        ssm = ts.LinearStateSpaceModel(hidden, (cu(Ao), cu(bo), cu(so)), torch.Size([o]))
        p = proposals.LinearGaussianObservations() if prop == "lgo" else proposals.Bootstrap()
        filt = SISR(ssm, 65536, proposal=p, ess_threshold=0.5, seed=1000 + seed)
        torch.manual_seed(seed)
        res = filt.batch_filter(y.cuda(), bar=False)
        lls.append(float(res.loglikelihood))
        means.append(res.filter_means[1:].cpu().double())
    lls, means = torch.tensor(lls, dtype=torch.float64), torch.stack(means)
    se_ll = lls.std() / math.sqrt(8)
    assert abs(lls.mean() - kll) <= 4.0 * se_ll + 1e-6, (lls.mean().item(), kll, se_ll.item())
    se_m = means.std(0) / math.sqrt(8)
    zs = (means.mean(0) - km) / (se_m + 1e-12)
    assert zs.abs().max() <= 12.0 and zs.square().mean() <= 3.0, (zs.abs().max().item(), zs.square().mean().item())


# ------------------------------------------------------------------------------------------------------- theta on the batch dim
def test_three_parameter_rows_batched_equal_three_unbatched_runs():
    from torch.distributions import Independent, Normal

    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.filters.particle import APF, proposals
    from pyfilter_amd.timeseries import LinearModel

    g = LC.load("cv4d_apf_lgo", "f64")
    d, o, n, B = 4, 2, 512, 3
    A = torch.stack([g["hid_A"].double() * f for f in (1.0, 0.97, 0.94)]).cuda()  # (B, D, D)
    s = torch.stack([g["hid_s"].double() * f for f in (1.0, 1.5, 2.0)]).cuda()     # (B, D)
    off, Ao, bo, so = (g[k].double().cuda() for k in ("hid_b", "obs_A", "obs_b", "obs_s"))
    y = g["y"].double().cuda()
    gen = torch.Generator().manual_seed(3)
    z = torch.randn((y.shape[0], n, B, d), generator=gen, dtype=torch.float64)
    u = torch.rand((y.shape[0], B), generator=gen, dtype=torch.float64)
    x0 = torch.randn((n, B, d), generator=gen, dtype=torch.float64)

    def run(a_, s_, cols):
        inc = Independent(Normal(torch.tensor(0.0, dtype=torch.float64, device="cuda"), torch.tensor(1.0, dtype=torch.float64, device="cuda"))
                          .expand(torch.Size([d])), 1)
        hidden = LinearModel((a_, off, s_), inc, lambda *_: Independent(Normal(torch.zeros(d, dtype=torch.float64, device="cuda"),
                                                                               torch.ones(d, dtype=torch.float64, device="cuda")), 1))
        filt = APF(ts.LinearStateSpaceModel(hidden, (Ao, bo, so), torch.Size([o])), n, proposal=proposals.LinearGaussianObservations())
        filt.set_batch_shape(torch.Size([len(cols)]))
        filt.set_tape(z=z[:, :, cols].contiguous(), u=u[:, cols].contiguous())
        st = filt.initialize()
        st["_x"] = st["_x"].copy(values=x0[:, cols].cuda().contiguous())
        for k in ("_mean", "_var"):
            st.pop(k, None)
        return filt.batch_filter(y, bar=False, init_state=st)

    whole = run(A, s, [0, 1, 2])
    for i in range(B):
        one = run(A[i:i + 1], s[i:i + 1], [i])
        torch.testing.assert_close(whole.loglikelihood[i:i + 1], one.loglikelihood, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(whole.filter_means[:, i:i + 1], one.filter_means, rtol=1e-12, atol=1e-12)


def test_smc2_fits_the_transition_scale_of_a_linear_model():
    from torch.distributions import Independent, Normal, Uniform

    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.filters.particle import APF, proposals
    from pyfilter_amd.inference import SMC2
    from pyfilter_amd.timeseries import LinearModel

    g = LC.load("cv4d_apf_lgo", "f64")
    d, o = 4, 2
    A, off, Ao, bo, so = (g[k].float().cuda() for k in ("hid_A", "hid_b", "obs_A", "obs_b", "obs_s"))
    y = g["y"].float().cuda()

    def build(theta):
        s = theta["sigma"].unsqueeze(-1).expand(-1, d)  # (B, D): one transition-scale row per theta-particle
        inc = Independent(Normal(torch.tensor(0.0, device="cuda"), torch.tensor(1.0, device="cuda")).expand(torch.Size([d])), 1)
        hidden = LinearModel((A, off, s), inc, lambda *_: Independent(Normal(torch.zeros(d, device="cuda"), torch.ones(d, device="cuda")), 1))
        return ts.LinearStateSpaceModel(hidden, (Ao, bo, so), torch.Size([o]))

    filt = APF(build, 256, proposal=proposals.LinearGaussianObservations(), seed=1)
    alg = SMC2(filt, 64, {"sigma": Uniform(0.01, 0.5)}, threshold=0.5, device=y.device, seed=2)
    state = alg.fit(y)
    mean = alg.posterior_mean(state)
    assert torch.isfinite(mean).all() and torch.isfinite(state.filter_state.loglikelihood).all()
    assert 0.01 <= float(mean.reshape(-1)[0]) <= 0.5
