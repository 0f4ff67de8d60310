"""TEST INFRASTRUCTURE - inputs of the nested-proposal kernel tests (``tests/test_nested_gpu.py``): single ``sample_and_weight``
calls on given parents, normals and uniforms, either teacher-forced from the float32 fixtures (``tools/make_golden_nested.py``)
or synthetic, each with its float64 oracle result (``tests/nested_oracle.py``) computed from the SAME (rounded) inputs."""
import math

import torch

from oracle import models as M
from oracle.cases import build_spec
from tests import nested_oracle
from tests.helpers import load_golden
from tools.make_golden_nested import CASE_BY_NAME, CASES

MODEL_CASE = {c["model"]: c for c in CASES}  # one fixture case per model: sv_batched, sine, lorenz, rw2d


def rounded_spec(case, dtype):
    """The case's model in float64 arithmetic with its parameters as a run in ``dtype`` holds them (rounded to it)."""
    spec = build_spec(case, dtype)
    r = lambda p: torch.as_tensor(p, dtype=dtype).double()  # noqa: E731
    spec.hidden_params = tuple(r(p) for p in spec.hidden_params)
    spec.obs_params = tuple(r(p) for p in spec.obs_params)
    return spec


class Call:
    """One call: ``x (N, B, [D])`` parents, ``y``, ``z (M, N, B, [D])``, ``v (N, B)`` in ``dtype`` (CPU) and the oracle's float64
    ``(x, w, pick)`` for them."""

    def __init__(self, name, case, dtype, x, y, z, v):
        self.name, self.case, self.dtype = name, case, dtype
        self.x, self.y, self.z, self.v = x, y, z, v
        self.m, self.n, self.b = z.shape[0], x.shape[0], x.shape[1]
        spec = rounded_spec(case, dtype)
        self.ref_x, self.ref_w, self.ref_pick = nested_oracle.nested_sample_and_weight(spec, y.double(), x.double(), z.double(), v.double())


def teacher_forced(dt="f32"):
    """Every weighted step of the fixtures of type ``dt``: the step's incoming particles, its normals and uniforms."""
    dtype = {"f32": torch.float32, "f64": torch.float64}[dt]
    calls = []
    for case in CASES:
        if dt not in case["dtypes"]:
            continue
        g = load_golden(case["name"], dt)
        xs = [g["x0"]] + list(g["step_x"].unbind(0))
        for t in range(case["T"]):
            if bool(g["y"][t].isnan().all()):
                continue
            calls.append(Call(f"{case['name']}[{t}]", case, dtype, xs[t].to(dtype), g["y"][t].to(dtype), g["z_tape"][t].to(dtype),
                              g["v_tape"][t].to(dtype)))
    return calls


def synthetic(model, n, b, m, dtype, seed=0, shared_y=None, negative_third=False):
    """Parents from the model's initial law, one transition on; ``y`` simulated from the first particle (one row per filter
    for the stochastic-volatility model unless ``shared_y``); float32 draws as in the fixtures.  ``negative_third``: every third
    parent negated (a stochastic-volatility parent < 0 has no valid candidate: the transition scale is sigma x)."""
    case = dict(MODEL_CASE[model], N=n, B=b)
    spec = build_spec(case, torch.float64)
    gen = torch.Generator().manual_seed(1000 + seed)
    tail = (spec.dim,) if spec.dim > 0 else ()
    rn = lambda *s: torch.randn(s, generator=gen, dtype=torch.float32).double()  # noqa: E731
    x = M.propagate(spec, M.initial_sample(spec, rn(n, b, *tail)), rn(n, b, *tail))
    loc, scale = M.obs_loc_scale(spec, M.propagate(spec, x[:1], rn(1, b, *tail)))
    y = (loc + M._t(scale, loc) * rn(*loc.shape))[0]  # (B, [O])
    per_filter = model == "sv_batched" if shared_y is None else not shared_y
    if not per_filter:
        y = y[0]
    if negative_third:
        x[::3] = -x[::3].abs()
    z = torch.randn((m, n, b) + tail, generator=gen, dtype=torch.float32)
    v = torch.rand((n, b), generator=gen, dtype=torch.float32)
    return Call(f"{model} {n}x{b} M={m}", case, dtype, x.to(dtype), y.to(dtype), z.to(dtype), v.to(dtype))


def last_candidate_invalid(dtype, n=200, b=2, m=6):
    """A stochastic-volatility call whose LAST candidate is invalid for every particle (its normal is -50: a negative candidate)
    and whose uniforms are 1: no running sum exceeds ``v sum``, so the pick falls to the last candidate of positive weight."""
    c = synthetic("sv_batched", n, b, m, dtype, seed=6)
    z, v = c.z.clone(), torch.ones_like(c.v)
    z[-1] = -50.0
    return Call(f"sv last candidate invalid {n}x{b} M={m}", c.case, dtype, c.x, c.y, z, v)


def f32_inputs():
    """The inputs the float32 bar is measured and checked on: every weighted step of the float32 fixtures and one synthetic call
    of at least 20 000 particles per model."""
    return teacher_forced("f32") + [synthetic("sv_batched", 5003, 4, 64, torch.float32), synthetic("sine", 10007, 2, 16, torch.float32),
                                    synthetic("lorenz", 10007, 2, 6, torch.float32), synthetic("rw2d", 10007, 2, 4, torch.float32)]


def weight_error(w, ref_w):
    """max ``|dw| / (1 + |w|)`` over the rows whose oracle weight is finite; the rows where it is -inf must be -inf."""
    w, dead = w.double().cpu(), ref_w == -math.inf
    assert bool((w[dead] == -math.inf).all()), "a particle without a valid candidate must weigh -inf"
    live = ~dead
    assert bool(w[live].isfinite().all())
    return float(((w[live] - ref_w[live]).abs() / (1.0 + ref_w[live].abs())).max()) if bool(live.any()) else 0.0


def pick_mismatch(pick, ref_pick):
    return float((pick.cpu().long() != ref_pick).double().mean())


def torch_route(call, device="cpu"):
    """The package's torch route (``NestedProposal.sample_and_weight`` without kernels) on the call's inputs, in its dtype."""
    from pyfilter_amd.filters.particle import proposals
    from pyfilter_amd.filters.particle.state import ParticleFilterPrediction
    from pyfilter_amd.timeseries import TimeseriesState
    from tests.helpers import build_ssm_from_case

    ssm = build_ssm_from_case(call.case, call.dtype, device)
    prop = proposals.NestedProposal(call.m).set_model(ssm)
    prop.record_picks = True
    x = call.x.to(device)
    prop.set_tape(z=call.z.unsqueeze(0).to(device), v=call.v.unsqueeze(0).to(device))
    state = TimeseriesState(0, x, ssm.hidden.event_shape)
    like = x[..., 0] if ssm.hidden.n_dim > 0 else x
    new, w = prop.sample_and_weight(call.y.to(device), ParticleFilterPrediction.equally_weighted(state, like))
    return new.value, w, prop.last_pick


def kernel_context(case, b, n, m, dtype):
    """(kind, packed parameter rows) of the case's model for ``b`` filters, through the filter's own packing."""
    from pyfilter_amd.filters.particle import SISR, proposals
    from tests.helpers import build_ssm_from_case

    ssm = build_ssm_from_case(dict(case, B=b), dtype, "cuda")
    filt = SISR(ssm, n, proposal=proposals.NestedProposal(m))
    filt.set_batch_shape(torch.Size([b]))
    ctx = filt._ensure_context()
    return ctx.kind, ctx.params, ssm.hidden.n_dim > 0


def run_kernel(call, z=True, seed=7, step=3):
    """The kernel (``pf_nested_sample_and_weight``) on the call's inputs - ``z = False``: on its own Philox draws - as CPU tensors in the
    reference's layout: (kept candidates, weights, picks)."""
    kind, params, has_event = kernel_context(call.case, call.b, call.n, call.m, call.dtype)
    from pyfilter_amd import ops
    from pyfilter_amd.filters.particle.proposals import NestedProposal

    soa = ops.to_soa(call.x.cuda(), True, has_event)
    zs = NestedProposal._candidates_soa(call.z.cuda(), True, has_event) if z else None
    vs = ops.to_cols(call.v.cuda()) if z else None
    x_out, w, pick = ops.nested_sample_and_weight_soa(kind, params, call.m, soa, call.y.cuda(), zs, vs, seed, step, want_pick=True)
    torch.cuda.synchronize()
    return ops.from_soa(x_out, True, has_event).cpu(), w.t().cpu(), pick.t().cpu().long()
