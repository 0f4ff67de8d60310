"""
Development (no GPU): writes ``tests/golden/{cv4d,lm6d,lm8d,rw5d}_*.npz`` - fixtures of linear-Gaussian models of 4 to 8 state
components, recorded from the unmodified reference run behind ``oracle/ref_shim`` (the shim's ``LinearModel``), with the tape
scheme of ``oracle/make_golden.py``: ``torch.normal`` and ``MultivariateNormal._standard_normal`` are wrapped to record the
standard normals ``z`` (drawn in float32, as there), a recording resampler records the systematic offsets ``u``.

    python tools/make_golden_linear.py          # needs the reference tree next to this repository's development box

===================  =====  ======================  =============  ==================================================
case                 D / O  filter, proposal        N x B x T      notes
===================  =====  ======================  =============  ==================================================
``cv4d_sisr_boot``   4 / 2  SISR, Bootstrap         256 x 2 x 20   constant-velocity tracker; observation 7 is NaN
``cv4d_apf_lgo``     4 / 2  APF, LGO                256 x 2 x 20   ``smooth(states, "fl")`` recorded
``lm6d_sisr_lgo``    6 / 4  SISR, LGO               200 x 3 x 15   dense stable A, one transition-scale row per filter
``lm8d_apf_boot``    8 / 8  APF, Bootstrap          128 x 1 x 12   dense observation matrix
``rw5d_sisr_lgo``    5 / 3  SISR, LGO               200 x 2 x 15   ``LinearModel(eye(5), sigma)`` - RandomWalk(dim=5)
===================  =====  ======================  =============  ==================================================

Each case is written in float64; the two ``cv4d`` cases in float32 too.  The model's parameters travel in the fixture
(``hid_A, hid_b, hid_s, obs_A, obs_b, obs_s, init_m, init_s``) so a test rebuilds exactly the model that ran.  Every
combination of the table runs on the reference; none had to be dropped.  The fixtures are data only.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")
REFERENCE = os.environ.get("PF_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))

CV_A = [[1.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]  # dt = 1

CASES = [
    dict(name="cv4d_sisr_boot", D=4, O=2, filter="sisr", proposal="bootstrap", N=256, B=2, T=20, seed=401, nan_rows=(7,),
         dtypes=("f64", "f32"), ess=0.7),
    dict(name="cv4d_apf_lgo", D=4, O=2, filter="apf", proposal="lgo", N=256, B=2, T=20, seed=402, nan_rows=(), dtypes=("f64", "f32"),
         ess=0.7, smooth=True),
    dict(name="lm6d_sisr_lgo", D=6, O=4, filter="sisr", proposal="lgo", N=200, B=3, T=15, seed=403, nan_rows=(), dtypes=("f64",),
         ess=0.7),
    dict(name="lm8d_apf_boot", D=8, O=8, filter="apf", proposal="bootstrap", N=128, B=1, T=12, seed=404, nan_rows=(), dtypes=("f64",),
         ess=0.7),
    dict(name="rw5d_sisr_lgo", D=5, O=3, filter="sisr", proposal="lgo", N=200, B=2, T=15, seed=405, nan_rows=(), dtypes=("f64",),
         ess=0.7),
]


def model_params(case):
    """float64 parameters of a case: (A, b, s, A_obs, b_obs, s_obs, m0, s0) - s of shape (D,) or (B, D)."""
    import torch

    g = torch.Generator().manual_seed(case["seed"])
    d, o, b = case["D"], case["O"], case["B"]
    n = case["name"]
    if n.startswith("cv4d"):
        A = torch.tensor(CV_A, dtype=torch.float64)
        off = torch.tensor([0.1, -0.05, 0.01, 0.02], dtype=torch.float64)
        s = torch.tensor([0.1, 0.15, 0.05, 0.08], dtype=torch.float64)
        Ao = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]], dtype=torch.float64)
        bo = torch.tensor([0.2, -0.1], dtype=torch.float64)
        so = torch.tensor([0.3, 0.25], dtype=torch.float64)
        m0 = torch.zeros(d, dtype=torch.float64)
        s0 = torch.tensor([1.0, 1.0, 0.5, 0.5], dtype=torch.float64)
    elif n.startswith("rw5d"):
        A = torch.eye(d, dtype=torch.float64)
        off = torch.zeros(d, dtype=torch.float64)
        s = torch.tensor([0.05, 0.1, 0.08, 0.12, 0.06], dtype=torch.float64)
        Ao = torch.randn(o, d, generator=g, dtype=torch.float64) * 0.6
        bo = torch.randn(o, generator=g, dtype=torch.float64) * 0.1
        so = torch.tensor([0.2, 0.25, 0.3], dtype=torch.float64)
        m0 = torch.zeros(d, dtype=torch.float64)
        s0 = s.clone()
    else:
        A = 0.6 * torch.eye(d, dtype=torch.float64) + 0.25 * torch.randn(d, d, generator=g, dtype=torch.float64) / d ** 0.5
        assert torch.linalg.eigvals(A).abs().max() < 1.0
        off = 0.1 * torch.randn(d, generator=g, dtype=torch.float64)
        s = 0.1 + 0.1 * torch.rand(d, generator=g, dtype=torch.float64)
        if b > 1:  # one row of transition scales per filter
            s = s * (1.0 + 0.25 * torch.arange(b, dtype=torch.float64)).unsqueeze(-1)
        Ao = torch.randn(o, d, generator=g, dtype=torch.float64) * 0.5
        if o == d:
            Ao = Ao + torch.eye(d, dtype=torch.float64)
        bo = 0.1 * torch.randn(o, generator=g, dtype=torch.float64)
        so = 0.2 + 0.2 * torch.rand(o, generator=g, dtype=torch.float64)
        m0 = torch.zeros(d, dtype=torch.float64)
        s0 = 0.5 * torch.ones(d, dtype=torch.float64)
    return A, off, s, Ao, bo, so, m0, s0


def simulate(case, params):
    """One observation series (T, O), float64, from the model itself (the first filter's parameter row)."""
    import torch

    A, off, s, Ao, bo, so, m0, s0 = params
    g = torch.Generator().manual_seed(case["seed"] + 1000)
    s1 = s if s.dim() == 1 else s[0]
    x = m0 + s0 * torch.randn(case["D"], generator=g, dtype=torch.float64)
    ys = []
    for t in range(case["T"]):
        x = off + A @ x + s1 * torch.randn(case["D"], generator=g, dtype=torch.float64)
        y = bo + Ao @ x + so * torch.randn(case["O"], generator=g, dtype=torch.float64)
        if t in case["nan_rows"]:
            y = torch.full_like(y, float("nan"))
        ys.append(y)
    return torch.stack(ys)


def _main_child(dtype_name: str):
    import numpy as np
    import torch

    dtype = {"f64": torch.float64, "f32": torch.float32}[dtype_name]
    torch.set_default_dtype(dtype)
    sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shim"))
    sys.path.insert(1, REFERENCE)

    import torch.distributions.multivariate_normal as mvn_mod
    from pyfilter.filters.particle import APF, SISR, proposals
    from pyfilter.resampling import systematic as ref_systematic
    from pyfilter.utils import get_ess as ref_get_ess, normalize as ref_normalize
    from stochproc import timeseries as ts
    from torch.distributions import Independent, Normal

    # the taping of oracle/make_golden.py: the draws are recorded, the reference's arithmetic is untouched
    class Tape:
        z, cur_u, mask = [], None, None

    tape = Tape()
    real_normal = torch.normal

    def taped_normal(mean, std, *args, **kwargs):
        if not (isinstance(mean, torch.Tensor) and isinstance(std, torch.Tensor)):
            return real_normal(mean, std, *args, **kwargs)
        z32 = torch.randn(mean.shape, dtype=torch.float32)
        tape.z.append(z32)
        return z32.to(mean.dtype) * std + mean

    def taped_standard_normal(shape, dtype, device):
        z32 = torch.randn(shape, dtype=torch.float32)
        tape.z.append(z32)
        return z32.to(dtype)

    torch.normal = taped_normal
    mvn_mod._standard_normal = taped_standard_normal

    os.makedirs(GOLDEN, exist_ok=True)
    for case in CASES:
        if dtype_name not in case["dtypes"]:
            continue
        params64 = model_params(case)
        y = simulate(case, params64).to(dtype)
        A, off, s, Ao, bo, so, m0, s0 = (p.to(dtype) for p in params64)
        d, n, b, t_len = case["D"], case["N"], case["B"], case["T"]
        torch.manual_seed(case["seed"])

        def init_kernel(*_):
            return Independent(Normal(m0, s0), 1)

        inc = Independent(Normal(torch.tensor(0.0), torch.tensor(1.0)).expand(torch.Size([d])), 1)
        hidden = ts.LinearModel((A, off, s), inc, init_kernel)
        ssm = ts.LinearStateSpaceModel(hidden, (Ao, bo, so), torch.Size([case["O"]]))

        filt_cls = {"sisr": SISR, "apf": APF}[case["filter"]]

        class Taped(filt_cls):
            def predict(self, state):
                if case["filter"] == "sisr":
                    w_ = ref_normalize(state.weights.clone())
                    tape.mask = ref_get_ess(w_, normalized=True) < self._resample_threshold
                else:
                    tape.mask = torch.ones(b, dtype=torch.bool)
                return super().predict(state)

        def taped_resampler(w, normalized=False):
            u = tape.cur_u[tape.mask].reshape(-1, 1).to(w.dtype)
            return ref_systematic(w, normalized=normalized, u=u)

        prop = {"bootstrap": proposals.Bootstrap, "lgo": proposals.LinearGaussianObservations}[case["proposal"]]()
        filt = Taped(ssm, n, resampling=taped_resampler, proposal=prop, ess_threshold=case["ess"])
        filt.set_batch_shape(torch.Size([b]))

        tape.z.clear()
        state = filt.initialize()
        z0 = tape.z.pop()
        assert not tape.z
        x0 = state.timeseries_state.value.clone()
        result = filt.initialize_with_result(state)
        steps = {k: [] for k in ("x", "w", "ll", "idx")}
        u_tape, z_tape, all_states = [], [], [state]
        for t in range(t_len):
            tape.cur_u = torch.rand(b, dtype=torch.float32)
            u_tape.append(tape.cur_u)
            state = filt.filter(y[t], state, result=result)
            _ = state.timeseries_state.value  # (the lazy sample)
            assert len(tape.z) == 1, len(tape.z)
            z_tape.append(tape.z.pop())
            steps["x"].append(state.timeseries_state.value.clone())
            steps["w"].append(state.weights.clone())
            steps["ll"].append(state.get_loglikelihood().clone())
            steps["idx"].append(state.previous_indices.clone())
            all_states.append(state)

        out = {
            "y": y.numpy(), "x0": x0.numpy(), "z0": z0.numpy(),
            "z_tape": torch.stack(z_tape).numpy(), "u_tape": torch.stack(u_tape).numpy(),
            "filter_means": result.filter_means.numpy(), "filter_variance": result.filter_variance.numpy(),
            "loglikelihood": result.loglikelihood.numpy(),
        }
        for k, v in steps.items():
            out[f"step_{k}"] = torch.stack(v).numpy()
        if case.get("smooth"):
            out["smooth_fl"] = filt.smooth(all_states, "fl").numpy()
        for k, v in zip(("hid_A", "hid_b", "hid_s", "obs_A", "obs_b", "obs_s", "init_m", "init_s"), params64):
            out[k] = v.numpy()
        path = os.path.join(GOLDEN, f"{case['name']}_{dtype_name}.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({os.path.getsize(path)} bytes): ll={result.loglikelihood.tolist()}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        _main_child(sys.argv[2])
    else:
        for dt in ("f64", "f32"):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", dt], cwd=ROOT)
