"""
Development (no GPU): writes ``tests/golden/nested_*.npz`` - SISR / APF runs of the unmodified reference with its
``NestedProposal(num_samples)`` (``proposals/nested.py``), imported behind ``oracle/ref_shim``; the models and observation
series are those of ``oracle.cases`` (``build_spec`` / ``simulate``).

    python tools/make_golden_nested.py          # needs the reference tree next to this repository's development box

Tape scheme (the reference's arithmetic is untouched; draw order per move: resampling ``u``, the candidates' normals, the pick):

* ``torch.normal`` is wrapped as in ``oracle/make_golden.py``: ``z = randn(shape)`` in float32, recorded.  A weighted move
  draws ONE ``(M, N, B, [D])`` block - row ``t`` of ``z_tape (T, M, N, B, [D])``; a propagate-only move (NaN observation)
  draws ``(N, B, [D])``, stored as ``z_tape[t, 0]`` (the other rows of that step are zero).
* a recording resampler draws the systematic offsets ``u_tape (T, B)`` (float32).
* the ``Categorical`` the proposal picks with is replaced, for the run, by one whose ``sample()`` draws ``v ~ U(0, 1)``
  (float32, one per particle: ``v_tape (T, N, B)``) and returns the inverse-CDF index ``(cumsum(probs, -1) < v).sum(-1)`` clamped to
  ``M - 1`` - the law of the ``torch.multinomial`` it stands in for, from an injectable draw.

Per case: ``y, x0, z0, z_tape, u_tape, v_tape``, per step the reference's ``step_x, step_w, step_ll, step_idx`` and
``step_pick`` (``-1`` on propagate-only moves), and ``filter_means, filter_variance, loglikelihood``; ``num_samples``.

====================  ===========  ================  ===  =============  =========
case                  model        filter            M    N x B x T      dtypes
====================  ===========  ================  ===  =============  =========
nested_sv_sisr        sv_batched   SISR, ess 0.6     8    256 x 4 x 12   f64, f32
nested_sv_apf         sv_batched   APF               5    200 x 3 x 12   f64
nested_sine_sisr_nan  sine         SISR, ess 0.9     16   300 x 2 x 12   f64, f32   (NaN at steps 3, 4)
nested_lorenz_sisr    lorenz       SISR, ess 0.9     6    128 x 2 x 8    f64
nested_rw2d_apf       rw2d         APF               4    256 x 3 x 10   f64, f32
====================  ===========  ================  ===  =============  =========

The fixtures are data only.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")
REFERENCE = os.environ.get("PF_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))

CASES = [
    dict(name="nested_sv_sisr", model="sv_batched", filter="sisr", M=8, N=256, B=4, T=12, ess_threshold=0.6, seed=501,
         dtypes=("f64", "f32")),
    dict(name="nested_sv_apf", model="sv_batched", filter="apf", M=5, N=200, B=3, T=12, ess_threshold=0.9, seed=502,
         dtypes=("f64",)),
    dict(name="nested_sine_sisr_nan", model="sine", filter="sisr", M=16, N=300, B=2, T=12, ess_threshold=0.9, seed=503,
         nan_steps=(3, 4), dtypes=("f64", "f32")),
    dict(name="nested_lorenz_sisr", model="lorenz", filter="sisr", M=6, N=128, B=2, T=8, ess_threshold=0.9, seed=504,
         dtypes=("f64",)),
    dict(name="nested_rw2d_apf", model="rw2d", filter="apf", M=4, N=256, B=3, T=10, ess_threshold=0.9, seed=505,
         dtypes=("f64", "f32")),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}


def _main_child(dtype_name: str):
    import numpy as np
    import torch

    dtype = {"f64": torch.float64, "f32": torch.float32}[dtype_name]
    torch.set_default_dtype(dtype)
    sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shim"))
    sys.path.insert(1, REFERENCE)
    sys.path.insert(2, ROOT)

    from pyfilter.filters.particle import APF, SISR, proposals
    from pyfilter.filters.particle.proposals import nested as ref_nested
    from pyfilter.resampling import systematic as ref_systematic
    from pyfilter.utils import get_ess as ref_get_ess, normalize as ref_normalize
    from stochproc import timeseries as ts
    from torch.distributions import Categorical, Independent, Normal

    from oracle import models as M
    from oracle.cases import build_spec, simulate

    class Tape:
        z, v, picks, cur_u, mask = [], [], [], None, None

    tape = Tape()
    real_normal = torch.normal

    def taped_normal(mean, std, *args, **kwargs):
        if not (isinstance(mean, torch.Tensor) and isinstance(std, torch.Tensor)):
            return real_normal(mean, std, *args, **kwargs)
        z32 = torch.randn(mean.shape, dtype=torch.float32)
        tape.z.append(z32)
        return z32.to(mean.dtype) * std + mean

    torch.normal = taped_normal

    class TapedCategorical(Categorical):
        def sample(self, sample_shape=torch.Size()):
            assert len(sample_shape) == 0
            p = self.probs  # (N, B, M)
            v32 = torch.rand(p.shape[:-1], dtype=torch.float32)
            tape.v.append(v32)
            pick = (p.cumsum(-1) < v32.to(p.dtype).unsqueeze(-1)).sum(-1).clamp(max=p.shape[-1] - 1)
            tape.picks.append(pick.clone())
            return pick

    ref_nested.Categorical = TapedCategorical

    def build_reference_model(spec):
        """The shim-side model of a ModelSpec, as ``oracle/make_golden.py`` builds it (the four kinds of this table)."""
        k, d = spec.hidden, spec.dim
        hp = tuple(torch.as_tensor(p, dtype=dtype) for p in spec.hidden_params)
        m0, s0 = (torch.as_tensor(v, dtype=dtype) for v in spec.init)

        def init_kernel(*_):
            n = Normal(m0, s0)
            return Independent(n, 1) if d > 0 else n

        inc = Normal(torch.tensor(0.0), torch.tensor(spec.inc_scale))
        if d > 0:
            inc = Independent(inc.expand(torch.Size([d])), 1)
        if k == M.HID_LINEAR and d > 0:
            hidden = ts.LinearModel((torch.eye(d, dtype=dtype), hp[2]), inc, init_kernel)
        elif k == M.HID_SINE_EM:
            hidden = ts.AffineEulerMaruyama(lambda x, g, s: (torch.sin(x.value - g), s), hp, inc, spec.dt, init_kernel)
        elif k == M.HID_VERHULST_EM:
            hidden = ts.AffineEulerMaruyama(lambda x, ka, g, s: (ka * (g - x.value) * x.value, s * x.value), hp, inc, spec.dt,
                                            init_kernel)
        elif k == M.HID_LORENZ63_EM:

            def f(x, s, r, b, sigma):
                v = x.value
                return torch.stack((-s * (v[..., 0] - v[..., 1]), r * v[..., 0] - v[..., 1] - v[..., 0] * v[..., 2],
                                    v[..., 0] * v[..., 1] - b * v[..., 2]), dim=-1), sigma

            hidden = ts.AffineEulerMaruyama(f, hp, inc, spec.dt, init_kernel)
        else:
            raise NotImplementedError(k)
        op = tuple(torch.as_tensor(p, dtype=dtype) for p in spec.obs_params)
        if spec.obs == M.OBS_LINEAR:
            return ts.LinearStateSpaceModel(hidden, op, torch.Size([spec.obs_dim]) if spec.obs_dim > 0 else torch.Size([]))
        return ts.StateSpaceModel(hidden, lambda x, mu: Normal(mu, x.value), op)

    os.makedirs(GOLDEN, exist_ok=True)
    for case in CASES:
        if dtype_name not in case["dtypes"]:
            continue
        torch.manual_seed(case["seed"])
        spec = build_spec(case, dtype)
        ssm = build_reference_model(spec)
        n, b, t_len, m = case["N"], case["B"], case["T"], case["M"]
        y = simulate(case, spec, dtype)
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
            assert w.dim() == 2 and w.shape[1] == u.shape[0]
            return ref_systematic(w, normalized=normalized, u=u)

        filt = Taped(ssm, n, resampling=taped_resampler, proposal=proposals.NestedProposal(m), ess_threshold=case["ess_threshold"])
        filt.set_batch_shape(torch.Size([b]))

        tape.z.clear()
        state = filt.initialize()
        z0 = tape.z.pop()
        assert not tape.z
        x0 = state.timeseries_state.value.clone()
        result = filt.initialize_with_result(state)
        steps = {k: [] for k in ("x", "w", "ll", "idx", "pick")}
        u_tape, z_tape, v_tape = [], [], []
        d_tail = tuple(x0.shape[2:])
        for t in range(t_len):
            tape.cur_u = torch.rand(b, dtype=torch.float32)
            u_tape.append(tape.cur_u)
            state = filt.filter(y[t], state, result=result)
            _ = state.timeseries_state.value  # (the lazy sample of a propagate-only move)
            assert len(tape.z) == 1, len(tape.z)
            z = tape.z.pop()
            if bool(y[t].isnan().all()):
                assert tuple(z.shape) == (n, b) + d_tail and not tape.v
                full = torch.zeros((m, n, b) + d_tail, dtype=torch.float32)
                full[0] = z
                z_tape.append(full)
                v_tape.append(torch.zeros(n, b, dtype=torch.float32))
                steps["pick"].append(torch.full((n, b), -1, dtype=torch.int64))
            else:
                assert tuple(z.shape) == (m, n, b) + d_tail and len(tape.v) == 1
                z_tape.append(z)
                v_tape.append(tape.v.pop())
                steps["pick"].append(tape.picks.pop())
            steps["x"].append(state.timeseries_state.value.clone())
            steps["w"].append(state.weights.clone())
            steps["ll"].append(state.get_loglikelihood().clone())
            steps["idx"].append(state.previous_indices.clone())

        out = {
            "y": y.numpy(), "x0": x0.numpy(), "z0": z0.numpy(), "num_samples": np.asarray(m, dtype=np.int64),
            "z_tape": torch.stack(z_tape).numpy(), "u_tape": torch.stack(u_tape).numpy(), "v_tape": torch.stack(v_tape).numpy(),
            "filter_means": result.filter_means.numpy(), "filter_variance": result.filter_variance.numpy(),
            "loglikelihood": result.loglikelihood.numpy(),
        }
        for k, v in steps.items():
            out[f"step_{k}"] = torch.stack(v).numpy()
        out["step_idx"] = out["step_idx"].astype(np.int32)
        out["step_pick"] = out["step_pick"].astype(np.int16)
        path = os.path.join(GOLDEN, f"{case['name']}_{dtype_name}.npz")
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        assert size < (1 << 20), (path, size)
        print(f"wrote {path} ({size} bytes): ll={result.loglikelihood.tolist()}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        _main_child(sys.argv[2])
    else:
        for dt in ("f64", "f32"):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", dt], cwd=ROOT)
