"""The path score: the complete-data log-likelihood of smoothed trajectories and its gradient with respect to the parameters -
by Fisher's identity an estimate of the score of the marginal likelihood.  It is the expression the reference differentiates for
its gradient-based PMMH proposal (``_model_likelihood``, ``inference/batch/mcmc/proposals/gradient.py:9-32``; the same sums in
``particle/base.py:176-210``) without the prior, which the proposal adds:

    value = initial_distribution.log_prob(x_0).mean(0) + (log p(x_t | x_{t-1}) + log p(y_t | x_t)).sum(0).mean(0)

* a built-in model of up to three state / observation components on a GPU: ``pf_path_score`` (``csrc/pf_score.hpp``) - one
  streaming launch gives the transition / observation sums and their gradient with respect to the kernels' parameter rows; the
  step from rows to the caller's parameters is a vector-Jacobian product through the model builder and ``pack_params`` (torch
  autograd over ``(B, NP)`` tensors), the initial term one ``(N, B)`` evaluation;
* a ``LinearModel`` of up to eight components under a linear-Gaussian observation of up to eight, on a GPU:
  ``pf_path_score_linear`` (``csrc/pf_linear_smooth.hpp``) - the same scheme in that kind's row layout
  ``[A | b | s | A_o | b_o | s_o]``; the vector-Jacobian product goes through ``linear_rows`` (``pack_params``' branch of the kind);
* anything else (user callables, larger shapes, CPU tensors) or ``route="torch"``: torch autograd of the whole expression, the
  reference's arithmetic.

Two deviations from the reference's expression, on both routes: an observation that is NaN in all its elements
contributes no observation term, as the filters skip it (the reference's sum would be NaN); and the kernel route's outputs are
float64 whatever the paths' type.  A row NaN in only some elements makes the value and the gradient of the filters it belongs
to NaN."""
from typing import Mapping, Optional

import torch
from torch.distributions import AffineTransform, Independent, Normal, TransformedDistribution

from ... import _lib as L
from ... import ops
from ...timeseries import AffineProcess, TimeseriesState
from ...timeseries.models import pack_params
from .forecast import kind_has_kernel, linear_kind_has_kernel, tape_soa

ROUTES = ("auto", "kernel", "torch")


def kernel_applies(model, paths: torch.Tensor) -> bool:
    kind = getattr(model, "kernel_kind", None)
    return kind_has_kernel(kind, paths) or linear_kind_has_kernel(kind, paths)


def _normal_base(dist):
    base = dist.base_dist if isinstance(dist, Independent) else dist
    return base if isinstance(base, Normal) else None


def initial_term(hidden, x0: torch.Tensor) -> torch.Tensor:
    """``initial_distribution.log_prob(x_0).mean(0)``.  A built-in process keeps its Gaussian initial law as ``init_mean`` /
    ``init_scale``, which may live on the host while the parameters are on the device (``ParticleFilter.initialize`` allows for
    that): they are read from there and moved to the paths' device - the process itself is not touched."""
    if hasattr(hidden, "init_mean") and hasattr(hidden, "init_scale"):
        m, s = torch.broadcast_tensors(hidden.init_mean.to(x0.device), hidden.init_scale.to(x0.device))
        lp = Normal(m, s, validate_args=False).log_prob(x0)
        return (lp.sum(-1) if hidden.n_dim > 0 else lp).mean(0)
    return hidden.initial_distribution.log_prob(x0).mean(0)


def transition_density(hidden, x: TimeseriesState):
    """``hidden.build_density(x)`` - with Gaussian increments that were built on the host (as the built-in kinds build them) read on
    the device of ``x``, again without touching the process."""
    inc = getattr(hidden, "increment_distribution", None)
    base = _normal_base(inc) if isinstance(hidden, AffineProcess) and inc is not None else None
    if base is None or base.loc.device == x.value.device:
        return hidden.build_density(x)
    dev = x.value.device
    moved = Normal(base.loc.to(dev), base.scale.to(dev), validate_args=False)
    if isinstance(inc, Independent):
        moved = Independent(moved, inc.reinterpreted_batch_ndims, validate_args=False)
    loc, scale = hidden.mean_scale(x)
    return TransformedDistribution(moved, AffineTransform(loc, scale, event_dim=hidden.n_dim), validate_args=False)


def _observations(model, y: torch.Tensor, steps: int, batched: bool, like: torch.Tensor):
    """``y (S - 1, [By], [O])`` -> ``(y broadcastable against (S - 1, N, [B], [O]) with its all-NaN rows zeroed, their mask
    broadcastable against (S - 1, N, [B]))``."""
    ev = len(model.event_shape)
    y = y.to(device=like.device, dtype=like.dtype)
    if y.shape[0] != steps:
        raise L.PfAmdError(f"path_score: {steps + 1} states need {steps} observations, got {y.shape[0]}")
    per_filter = y.dim() - 1 - ev  # 0: one series shared by the filters; 1: one per filter
    if per_filter not in (0, 1) or (per_filter == 1 and not batched and y.shape[1] != 1):
        raise L.PfAmdError(f"path_score: observations of shape {tuple(y.shape)} do not broadcast against the filters")
    lead = (steps, 1) + ((y.shape[1] if per_filter else 1,) if batched else ())
    y = y.reshape(lead + tuple(y.shape[y.dim() - ev:]))
    missing = y.isnan().reshape(lead + (-1,)).all(-1)
    clean = torch.where(missing.reshape(lead + (1,) * ev), torch.zeros_like(y), y)
    return clean, missing


def torch_score(model, paths: torch.Tensor, y: torch.Tensor, batched: bool) -> torch.Tensor:
    """The expression as torch operations on the model's own densities (differentiable): ``([B],)``."""
    hidden = model.hidden
    s = paths.shape[0]
    time = torch.arange(s, device=paths.device)
    x_tm1 = TimeseriesState(time[:-1], paths[:-1], hidden.event_shape)
    x_t = TimeseriesState(time[1:], paths[1:], hidden.event_shape)
    clean, missing = _observations(model, y, s - 1, batched, paths)
    trans = transition_density(hidden, x_tm1).log_prob(paths[1:])
    obs = model.build_density(x_t).log_prob(clean)
    obs = torch.where(missing, torch.zeros_like(obs), obs)
    return initial_term(hidden, paths[0]) + (trans + obs).sum(0).mean(0)


def path_score(filter_, paths: torch.Tensor, y: torch.Tensor, theta: Optional[Mapping[str, torch.Tensor]] = None,
               route: str = "auto"):
    """``ParticleFilter.path_score`` (see there)."""
    if route not in ROUTES:
        raise ValueError(f"path_score: route must be one of {ROUTES}, got {route!r}")
    if paths.shape[0] < 2:
        raise L.PfAmdError("path_score: needs at least two states")
    batched = filter_._batched
    b = filter_.batch_shape[0] if batched else 1
    leaves = None
    if theta is None:
        model = filter_.ssm
    else:
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in theta.items()}
        model = filter_._model_builder(leaves)
    if int(model.observe_every_step) != 1:
        raise NotImplementedError("path_score: the expression assumes observe_every_step = 1")
    has_event = model.hidden.n_dim > 0
    on_kernel = route != "torch" and kernel_applies(model, paths)
    if route == "kernel" and not on_kernel:
        raise L.PfAmdError("path_score: no kernel for this model / device (built-in kinds with D, O <= 3 and LinearModel with "
                           "D, O <= 8 under a linear-Gaussian observation, on a GPU)")

    if not on_kernel:
        with torch.enable_grad() if leaves is not None else torch.no_grad():
            value = torch_score(model, paths, y, batched)
        if leaves is None:
            return value
        if value.requires_grad:
            value.backward(torch.ones_like(value))
        value = value.detach()
        poison = value * 0.0  # (NaN where the value is: a half-observed row - the kernel route's convention)
        grads = {}
        for k, leaf in leaves.items():
            g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
            per_filter = batched and g.dim() >= 1 and g.shape[0] == b
            grads[k] = g + (poison.reshape((b,) + (1,) * (g.dim() - 1)) if per_filter else poison.sum())
        return value, grads

    kind = model.kernel_kind
    dtype, device = paths.dtype, paths.device
    soa = tape_soa(paths, paths, batched, has_event)  # (S, D, B, N)
    with torch.enable_grad() if leaves is not None else torch.no_grad():
        rows = pack_params(model, b, dtype, device)
        init = initial_term(model.hidden, paths[0])
    run = ops.path_score_linear if kind.hid_kind == L.HID_LINEAR_MAT else ops.path_score
    sums, grad_rows = run(kind, rows.detach().contiguous(), soa, y)
    value = sums + init.detach().to(torch.float64).reshape(-1)
    value = value if batched else value[0]
    if leaves is None:
        return value
    outs = [(rows, grad_rows.to(rows.dtype)), (init, torch.ones_like(init))]
    outs = [(t, g) for t, g in outs if t.requires_grad]  # (one pass: the two may share a piece of the builder's graph)
    if outs:
        torch.autograd.backward([t for t, _ in outs], [g for _, g in outs])
    return value, {k: (leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)) for k, leaf in leaves.items()}
