"""Forecasting from a filter state: the weighted particles walked ``steps`` moves of the hidden process ahead, with the predictive
mean and variance of the state and of the observation at every one of them - what ``ParticleFilterCorrection.predict_path``
(``particle/state.py:173-174``) is used for, with three differences: the particle weights enter, the
observation's moments are Rao-Blackwellised (``sum W m(x)``, ``sum W (m(x)^2 + s(x)^2)`` from the observation density's
conditional mean and scale: no observation noise is drawn for them), and the draws are the filter's own (Philox keyed by a seed,
or tapes), not torch's global generator.

* a built-in model of up to three state / observation components on a GPU: ``pf_forecast`` (``csrc/pf_forecast.hpp``) - one launch
  for the whole horizon, nothing particle-sized written unless paths are asked for;
* a ``LinearModel`` (or a ``RandomWalk`` of four to eight dimensions: the same kind) of up to eight state / observation components
  under a linear-Gaussian observation on a GPU, when asked for with ``route="kernel"``: ``pf_forecast_linear``
  (``csrc/pf_forecast_linear.hpp``) - the same scheme, with predictive covariances as an option;
* anything else (user callables, ``LinearModel`` by default, a scalar state under a vector observation, CPU tensors, a built-in
  model's covariances): ``torch_forecast``, the same outputs from the same tapes as torch operations.

Moments follow ``get_filter_mean_and_variance``: weights are taken as normalised (no division by ``sum W``) and the variance is
``sum W (x - mean)^2`` - centred before squaring (the kernel: sums about a pivot), so a cloud far from zero keeps it.  Covariances
(``covariance=True``) follow the variances: ``sum W (x - mean)(x - mean)^T``, and for the observation the covariance of the
conditional means plus ``diag(sum W s(x)^2)``."""
from typing import Optional

import torch
from torch.distributions import Independent, Normal

from ... import _lib as L
from ... import ops
from ...timeseries import AffineProcess, StateSpacePath, TimeseriesState


class Forecast:
    """``x_mean``, ``x_variance``: ``(steps, [B], [D])``; ``y_mean``, ``y_variance``: ``(steps, [B], [O])``; ``paths``: a
    ``StateSpacePath`` in ``predict_path``'s layout - ``get_paths() -> (x (steps, N, [B], [D]), y (steps, N, [B], [O]))`` - or None;
    ``x_covariance (steps, [B], D, D)``, ``y_covariance (steps, [B], O, O)`` (a scalar state or observation: ``(..., 1, 1)``) or None."""

    def __init__(self, x_mean, x_variance, y_mean, y_variance, paths: Optional[StateSpacePath] = None, x_covariance=None,
                 y_covariance=None):
        self.x_mean, self.x_variance, self.y_mean, self.y_variance, self.paths = x_mean, x_variance, y_mean, y_variance, paths
        self.x_covariance, self.y_covariance = x_covariance, y_covariance

    def __repr__(self):
        return f"Forecast(steps: {self.x_mean.shape[0]}, x: {tuple(self.x_mean.shape[1:])}, y: {tuple(self.y_mean.shape[1:])}, " \
               f"paths: {self.paths is not None}, covariances: {self.x_covariance is not None})"


def mix_forecasts(w: torch.Tensor, fc: Forecast) -> Forecast:
    """The mixture of ``B`` filters' forecasts (moments ``(steps, B, ...)``) under the normalised weights ``w (B,)`` - the
    posterior predictive of SMC2 / NESS: ``mean = sum_b w_b mean_b``, ``var = sum_b w_b (var_b + (mean_b - mean)^2)`` (the members'
    means centred before squaring: no cancellation at a level far from zero) and, when the forecast has covariances,
    ``cov = sum_b w_b (cov_b + (mean_b - mean)(mean_b - mean)^T)``.  Evaluated in float64, returned in the forecasts' type."""
    def mix(mean, var):
        m, v = mean.double(), var.double()
        ww = w.to(device=m.device, dtype=torch.float64).reshape((1, -1) + (1,) * (m.dim() - 2))
        mu = (ww * m).sum(1)
        mixed = (ww * (v + (m - mu.unsqueeze(1)) ** 2)).sum(1)
        return mu.to(mean.dtype), mixed.clamp_min(0.0).to(var.dtype)

    def mix_cov(mean, cov):
        if cov is None:
            return None
        m = mean.double().reshape(cov.shape[:-1])  # (a scalar state's mean has no event dimension: (steps, B) -> (steps, B, 1))
        ww = w.to(device=m.device, dtype=torch.float64).reshape(1, -1, 1)
        dm = m - (ww * m).sum(1, keepdim=True)
        return (ww.unsqueeze(-1) * (cov.double() + dm.unsqueeze(-1) * dm.unsqueeze(-2))).sum(1).to(cov.dtype)

    xm, xv = mix(fc.x_mean, fc.x_variance)
    ym, yv = mix(fc.y_mean, fc.y_variance)
    return Forecast(xm, xv, ym, yv, None, mix_cov(fc.x_mean, fc.x_covariance), mix_cov(fc.y_mean, fc.y_covariance))


def normalized_weights(log_w: torch.Tensor) -> torch.Tensor:
    """``normalize`` of the log-weights ``(N, [B])`` WITHOUT its in-place sanitising of the argument (a forecast leaves the state
    as it found it); on a CPU the same as torch operations (NaN, +inf and -inf count as the lowest finite value's weight)."""
    if log_w.is_cuda:
        from ...utils import normalize

        return normalize(log_w.clone())
    low = torch.finfo(log_w.dtype).min
    lw = torch.nan_to_num(log_w, nan=low, posinf=low, neginf=low)
    return torch.softmax(lw - lw.max(dim=0, keepdim=True)[0], dim=0)


def kind_has_kernel(k, x: torch.Tensor) -> bool:
    """A built-in kind of the stand-alone model kernels with ``D, O <= 3``, tensors on a GPU (``pf_forecast``, ``pf_path_score``)."""
    if k is None or not x.is_cuda:
        return False
    return not k.is_user and k.hid_kind != L.HID_LINEAR_MAT and k.dim <= L.MAX_D and k.obs_dim is not None and k.obs_dim <= L.MAX_O


def linear_kind_has_kernel(k, x: torch.Tensor) -> bool:
    """``PF_HID_LINEAR_MAT`` (``LinearModel``) under a linear-Gaussian observation with ``D, O <= 8``, tensors on a GPU
    (``pf_path_score_linear``, ``pf_smooth_ffbs_linear``, ``pf_forecast_linear``)."""
    if k is None or not x.is_cuda:
        return False
    return (not k.is_user and k.hid_kind == L.HID_LINEAR_MAT and k.obs_kind == L.OBS_LINEAR and 1 <= k.dim <= L.LIN_MAX_D
            and k.obs_dim is not None and 1 <= k.obs_dim <= L.LIN_MAX_O)


def kernel_applies(ctx, x: torch.Tensor) -> bool:
    return ctx is not None and kind_has_kernel(ctx.kind, x)


def tape_soa(t: Optional[torch.Tensor], like: torch.Tensor, batched: bool, has_event: bool) -> Optional[torch.Tensor]:
    """``(steps, N, [B], [K])`` -> the kernel's ``(steps, K, B, N)``."""
    if t is None:
        return None
    t = t.to(device=like.device, dtype=like.dtype)
    if not has_event:
        t = t.unsqueeze(-1)
    if not batched:
        t = t.unsqueeze(2)
    return t.permute(0, 3, 2, 1).contiguous()


def _path_view(p: torch.Tensor, batched: bool, has_event: bool) -> torch.Tensor:
    """``(steps, K, B, N)`` -> the reference's ``(steps, N, [B], [K])`` view."""
    v = p.permute(0, 3, 2, 1)
    if not batched:
        v = v[:, :, 0]
    if not has_event:
        v = v[..., 0]
    return v


def kernel_forecast(ctx, obs_event: bool, x: TimeseriesState, w: Optional[torch.Tensor], steps: int, paths: bool,
                    z: Optional[torch.Tensor], e: Optional[torch.Tensor], seed: int) -> Forecast:
    """``pf_forecast`` on the reference-layout state ``x`` and normalised weights ``w (N, [B])``."""
    soa = ops.to_soa(x.value, ctx.batched, ctx.has_event)
    xm, xv, ym, yv, xp, yp = ops.forecast_soa(ctx.kind, ctx.params, steps, soa, None if w is None else ops.to_cols(w),
                                              tape_soa(z, soa, ctx.batched, ctx.has_event), tape_soa(e, soa, ctx.batched, obs_event),
                                              seed, paths)

    def shaped(m, event):
        m = m if ctx.batched else m[:, 0]
        return m if event else m[..., 0]

    path = StateSpacePath.from_tensors(_path_view(xp, ctx.batched, ctx.has_event), _path_view(yp, ctx.batched, obs_event)) if paths else None
    return Forecast(shaped(xm, ctx.has_event), shaped(xv, ctx.has_event), shaped(ym, obs_event), shaped(yv, obs_event), path)


def linear_kernel_forecast(ctx, obs_event: bool, x: TimeseriesState, w: Optional[torch.Tensor], steps: int, paths: bool,
                           z: Optional[torch.Tensor], e: Optional[torch.Tensor], seed: int, covariance: bool) -> Forecast:
    """``pf_forecast_linear`` on the reference-layout state ``x`` and normalised weights ``w (N, [B])``."""
    soa = ops.to_soa(x.value, ctx.batched, ctx.has_event)
    xm, xv, ym, yv, xc, yc, xp, yp = ops.forecast_linear_soa(
        ctx.kind, ctx.params, steps, soa, None if w is None else ops.to_cols(w), tape_soa(z, soa, ctx.batched, ctx.has_event),
        tape_soa(e, soa, ctx.batched, obs_event), seed, paths, covariance)

    def shaped(m, event):
        m = m if ctx.batched else m[:, 0]
        return m if event else m[..., 0]

    def batch(c):
        return None if c is None else (c if ctx.batched else c[:, 0])

    path = StateSpacePath.from_tensors(_path_view(xp, ctx.batched, ctx.has_event), _path_view(yp, ctx.batched, obs_event)) if paths else None
    return Forecast(shaped(xm, ctx.has_event), shaped(xv, ctx.has_event), shaped(ym, obs_event), shaped(yv, obs_event), path, batch(xc),
                    batch(yc))


def _weighted(w: torch.Tensor, first: torch.Tensor, within, dtype):
    """``(mu = sum W first, sum W ((first - mu)^2 + within))`` over dim 0 in float64 (``first`` float64; ``within``: a variance
    around ``first``, or 0.0) - centred before squaring, as ``get_filter_mean_and_variance``."""
    ww = w.double().reshape(w.shape + (1,) * (first.dim() - w.dim()))
    mu = (ww * first).sum(0)
    var = (ww * ((first - mu) ** 2 + within)).sum(0)
    return mu.to(dtype), var.clamp_min(0.0).to(dtype)


def _weighted_cov(w: torch.Tensor, first: torch.Tensor, within, event: bool, dtype):
    """``sum W (first - mu)(first - mu)^T + diag(sum W within)`` over dim 0 in float64, ``(..., K, K)`` (``first`` float64, ``(N, [B],
    [K])``: without an event dimension ``K = 1``) - centred before the outer product, as ``_weighted``."""
    if not event:
        first = first.unsqueeze(-1)
        within = within.unsqueeze(-1) if torch.is_tensor(within) else within
    ww = w.double().reshape(w.shape + (1,) * (first.dim() - w.dim()))
    c = first - (ww * first).sum(0)
    cov = (ww.unsqueeze(-1) * (c.unsqueeze(-1) * c.unsqueeze(-2))).sum(0)  # (c_i c_j first: both triangles get the same bits)
    if torch.is_tensor(within):
        cov = cov + torch.diag_embed((ww * within).sum(0))
    return cov.to(dtype)


def _normal_base(dist) -> Optional[Normal]:
    base = dist.base_dist if isinstance(dist, Independent) else dist
    return base if isinstance(base, Normal) else None


def torch_forecast(model, x: TimeseriesState, w: Optional[torch.Tensor], steps: int, paths: bool, z: Optional[torch.Tensor],
                   e: Optional[torch.Tensor], seed: int, covariance: bool = False) -> Forecast:
    """The same forecast as torch operations on the model's callables, on the device of ``x``.  ``z (steps, N, [B], [D])`` /
    ``e (steps, N, [B], [O])``: standard normals; without them the draws come from a ``torch.Generator`` seeded with ``seed``.
    An affine process with Gaussian increments moves by ``loc + scale * (increment scale * z)``; any other process moves by its
    own ``propagate`` (then a ``z`` tape is refused), and an observation density that is not Gaussian is sampled by its own
    ``sample``.  ``covariance``: the predictive covariances too (float64 sums, centred before the outer product)."""
    if steps < 1:
        raise L.PfAmdError("forecast: steps must be at least 1")
    hidden = model.hidden
    value = x.value
    dtype, device = value.dtype, value.device
    lead = value.dim() - len(x.event_shape)
    if w is None:
        w = torch.full(value.shape[:lead], 1.0 / value.shape[0], dtype=torch.float64, device=device)
    inc = getattr(hidden, "increment_distribution", None)
    base = _normal_base(inc) if isinstance(hidden, AffineProcess) and inc is not None else None
    kind = getattr(model, "kernel_kind", None)  # (its increment scale is a host double; the distribution's may be rounded)
    # two generators - transitions, observation noise: the same seed moves the particles alike with or without paths
    gen = torch.Generator(device=device).manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF) if z is None else None
    gen_e = torch.Generator(device=device).manual_seed((int(seed) ^ 0x5DEECE66D) & 0x7FFFFFFFFFFFFFFF) if paths and e is None else None
    rows = {k: [] for k in ("xm", "xv", "ym", "yv", "xc", "yc", "x", "y")}
    for h in range(steps):
        if base is not None:
            zh = z[h].to(device=device, dtype=dtype) if z is not None else torch.randn(value.shape, generator=gen, dtype=dtype, device=device)
            loc, scale = hidden.mean_scale(x)
            x = x.propagate_from(values=loc + scale * (zh * kind.inc_scale if kind is not None and not kind.is_user else base.loc + base.scale * zh))
        else:
            if z is not None:
                raise L.PfAmdError("a z tape needs an affine process with Gaussian increments")
            x = hidden.propagate(x)
        value = x.value
        dens = model.build_density(x)
        m, var = dens.mean, dens.variance
        m, var = torch.broadcast_tensors(m, var)
        xm, xv = _weighted(w, value.double(), 0.0, dtype)
        ym, yv = _weighted(w, m.double(), var.double(), dtype)
        for k, v in zip(("xm", "xv", "ym", "yv"), (xm, xv, ym, yv)):
            rows[k].append(v)
        if covariance:
            rows["xc"].append(_weighted_cov(w, value.double(), 0.0, len(x.event_shape) > 0, dtype))
            rows["yc"].append(_weighted_cov(w, m.double(), var.double(), m.dim() > lead, dtype))
        if paths:
            rows["x"].append(value)
            if _normal_base(dens) is not None:
                eh = e[h].to(device=device, dtype=dtype) if e is not None else torch.randn(m.shape, generator=gen_e, dtype=dtype, device=device)
                rows["y"].append(m + dens.stddev * eh)
            else:
                rows["y"].append(dens.sample())
    path = StateSpacePath(rows["x"], rows["y"]) if paths else None
    covs = [torch.stack(rows[k], 0) if covariance else None for k in ("xc", "yc")]
    return Forecast(*(torch.stack(rows[k], 0) for k in ("xm", "xv", "ym", "yv")), path, *covs)
