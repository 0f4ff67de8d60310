"""The backward-draw oracle (``oracle.cpu_ref.ffbs_backward_step``) and the inputs of the smoothing-kernel tests
(``tests/smoothing_cases.py``), without a GPU: the oracle's loop is the backward pass it replaced, its fallback rule, and the
conditions the GPU bars of ``tests/test_smoothing_kernels_gpu.py`` rest on."""
import math

import pytest
import torch

from oracle import cpu_ref
from oracle import models as M
from oracle.cases import CASE_BY_NAME, build_spec
from tests import smoothing_cases as sc
from tests.helpers import DT, load_golden


def _previous_smooth_ffbs(spec, xs, ws, start, u):
    """``cpu_ref.smooth_ffbs`` as it stood before ``ffbs_backward_step`` (kept here as the comparison)."""
    res = [start]
    for t in range(len(xs) - 2, -1, -1):
        logits = cpu_ref.ffbs_logits(spec, xs[t], ws[t], res[-1])  # (N_j, N_i, [B])
        if logits.dim() == 3:
            logits = logits.moveaxis(1, 2)  # (N_j, B, N_i)
        m = logits.max(dim=-1, keepdim=True)[0]
        e = (logits - m).exp().double()
        cdf = e.cumsum(dim=-1)
        target = u[t].double().unsqueeze(-1) * cdf[..., -1:]
        idx = (cdf > target).to(torch.int64).argmax(dim=-1)  # first candidate beyond the target
        x_t = xs[t]
        if spec.dim > 0:
            res.append(x_t.gather(0, idx.unsqueeze(-1).expand(idx.shape + (spec.dim,))))
        else:
            res.append(x_t.gather(0, idx))
    return torch.stack(res[::-1], dim=0)


@pytest.mark.parametrize("name", ["lg1d_sisr_boot", "rw2d_sisr_boot"])
def test_backward_step_loop_is_the_previous_backward_pass(name):
    case = CASE_BY_NAME[name]
    g = load_golden(name, "f64")
    spec = build_spec(case, torch.float64)
    n, b = case["N"], case["B"]
    xs = [g["x0"]] + list(g["step_x"].unbind(0))
    ws = [torch.zeros(n, b, dtype=torch.float64)] + list(g["step_w"].unbind(0))
    gen = torch.Generator().manual_seed(31)
    u = torch.rand((len(xs) - 1, n, b), generator=gen, dtype=torch.float64)
    start = xs[-1][torch.randint(n, (n,), generator=gen)]
    assert torch.equal(cpu_ref.smooth_ffbs(spec, xs, ws, start, u), _previous_smooth_ffbs(spec, xs, ws, start, u))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_backward_step_fallback_and_weight_rules(dt):
    """Three candidates at hand: u at 1 takes the last candidate of positive mass (the previous rule: candidate 0), u = 0 skips a
    leading candidate without mass; NaN, +inf, -inf and the dtype's lowest finite value are all without mass."""
    dtype = DT[dt]
    spec = build_spec(dict(model="lg1d", B=1), dtype)
    inf, low = math.inf, torch.finfo(dtype).min
    x_t = torch.tensor([[0.00], [0.01], [0.02]], dtype=dtype)
    x_next = torch.tensor([[0.01], [0.01], [0.01], [0.01]], dtype=dtype)
    u = torch.tensor([[0.0], [0.5], [1.0 - torch.finfo(dtype).eps], [1.0]], dtype=dtype)
    idx, cdf = cpu_ref.ffbs_backward_step(spec, x_t, torch.tensor([[-inf], [0.0], [-inf]], dtype=dtype), x_next, u)
    assert idx.dtype == torch.int64 and idx.shape == (4, 1) and cdf.dtype == torch.float64 and cdf.shape == (4, 1, 3)
    assert idx[:, 0].tolist() == [1, 1, 1, 1]  # (u = 0: not candidate 0; u = 1: candidate 1, not the trailing -inf one, not 0)
    assert torch.equal(cdf[0, 0], torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64))
    idx, _ = cpu_ref.ffbs_backward_step(spec, x_t, torch.tensor([[0.0], [0.0], [0.0]], dtype=dtype), x_next, u)
    assert idx[0, 0] == 0 and idx[3, 0] == 2
    for bad in (math.nan, inf, -inf, low):
        w = torch.tensor([[bad], [0.0], [bad]], dtype=dtype)
        idx, cdf = cpu_ref.ffbs_backward_step(spec, x_t, w, x_next, u)
        assert idx[:, 0].tolist() == [1, 1, 1, 1] and bool(cdf.isfinite().all()), bad
    assert torch.equal(cpu_ref.ffbs_sanitize_logw(torch.tensor([math.nan, inf, -inf, low, 1.5], dtype=dtype)),
                       torch.tensor([-inf, -inf, -inf, -inf, 1.5], dtype=dtype))


def _histories():
    return [("draws",) + c for c in sc.DRAW_CASES] + [("edges",) + c for c in sc.EDGE_CASES]


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("what,model,n,b,s", _histories(), ids=[f"{w}-{m}-{n}x{b}x{s}" for w, m, n, b, s in _histories()])
def test_input_conditions_of_the_gpu_bars(what, model, n, b, s, dt):
    """For every history the GPU tests run: distinct particles and a median of ``min_effective`` candidates per draw on the
    float64 oracle (asserted by ``synthetic``); in float32 the float32 oracle differs from the float64 oracle - both teacher-forced
    from the float64 picks - in at most 1e-3 of the draws, each within its own cdf error (factor 1) of a boundary."""
    dtype = DT[dt]
    h = sc.synthetic(model, n, b, s, dtype) if what == "draws" else sc.edge_history(model, n, b, s, dtype)
    assert h.s == s and h.n == n and h.b == b and len(h.logw) == s and h.u.shape == (max(s - 1, 0), n, b)
    assert all(x.dtype == dtype for x in h.x + h.logw + [h.x_last, h.u])
    if s == 1 or dtype == torch.float64:
        return
    ref = sc.oracle_pass(h, torch.float64)
    chain = lambda t: h.x_last if t == s - 1 else sc.gather(h.x[t], ref["idx"][t])  # noqa: E731
    low = sc.oracle_pass(h, torch.float32, x_next_of=chain)
    delta = sc.f32_delta(low, ref, 1.0)
    bad, total, worst = sc.compare_draws(h, low["idx"], ref, delta, f"{what} {model} {n}x{b}x{s}")
    print(f"float32 oracle, {what} {model} {n}x{b}x{s}: {bad} of {total} draws differ, distance {worst:.3e}, its cdf error {delta:.3e}")


def test_a_plain_lorenz_history_would_only_check_an_argmax():
    """Why the Lorenz kinds start from a tight cloud: from the model's initial law one candidate holds all of a draw's mass."""
    spec = build_spec(dict(model="lorenz", B=1), torch.float64)
    gen = torch.Generator().manual_seed(1)
    rn = lambda: torch.randn((300, 1, 3), generator=gen, dtype=torch.float64)  # noqa: E731
    x = M.initial_sample(spec, rn())
    for _ in range(3):
        x = M.propagate(spec, x, rn())
    nxt = M.propagate(spec, x[torch.randint(300, (300,), generator=gen)], rn())
    _, cdf = cpu_ref.ffbs_backward_step(spec, x, torch.zeros(300, 1, dtype=torch.float64), nxt, torch.zeros(300, 1, dtype=torch.float64))
    p = torch.diff(cdf, dim=-1, prepend=torch.zeros_like(cdf[..., :1]))
    assert (1.0 / p.pow(2).sum(-1)).median().item() < 1.5
