"""NESS (Crisan & Miguez' nested particle filter) - purely online parameter inference: theta-particles on the filters' batch
dimension, one fused ``filter()`` move per observation and, when the ESS of the theta-weights has dropped, an update that
resamples whole filters and *jitters* the parameters instead of re-filtering the data - a constant cost per observation.

Mirrors ``pyfilter/inference/sequential/ness.py:14-111`` (``BaseOnlineAlgorithm._step``, ``NESS``, ``FixedWidthNESS``),
``sequential/kernels/online.py:8-51`` (``OnlineKernel.update``) and ``sequential/kernels/jittering.py`` (``robust_var``, the
four kernel families) - with the reference's ``InferenceContext`` replaced by ``ThetaParticles``, as in ``SMC2``.

Two routes for the update's arithmetic.  Scalar priors of the native families on one GPU with at most ``_lib.JITTER_MAXB``
theta-particles: ``pf_theta_resample``, ``pf_jitter_fit`` and ``pf_jitter_apply`` (``csrc/pf_jitter.hpp``) - three launches,
the ancestors never leave the device.  Everything else (CPU tensors, other priors, more theta-particles,
``HINTS.theta_kernels = False``): the reference's torch operations restated below."""
import math
from typing import Optional, Tuple, Union

import torch

from .. import _lib
from ..hints import HINTS
from .parameters import ThetaParticles
from .pmmh import ThetaDraws, _to_device
from .smc2 import SMC2State, online_move, posterior_forecast
from .utils import theta_normalize, theta_systematic

INFTY = math.inf


class NessDraws(ThetaDraws):
    """The theta-level draws of an update in the reference's order: the resampling uniform (``online.py:33``), the jitter's
    standard normals (``jittering.py:26``) and - ``discrete`` - the Bernoulli draws (``online.py:39-43``).  ``taped``: the
    kernel route takes ``normal`` / ``bernoulli`` from here too (a parity run) instead of drawing them on the device."""

    taped = False

    def bernoulli(self, shape, p: float) -> torch.Tensor:
        return (torch.rand(tuple(shape), generator=self.generator, dtype=torch.float64) < p).double()


def _eps_of(dtype) -> float:
    """``pyfilter.constants.EPS`` for tensors of ``dtype`` (the reference evaluates it for the default dtype at import)."""
    return math.sqrt(torch.finfo(dtype).eps)


def robust_var(x: torch.Tensor, w: torch.Tensor, mean: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``V = min(IQR / 1.349, sigma)^2`` per column of ``x (B, P)`` under the normalised weights ``w (B,)``
    (``jittering.py:51-89``, restated).  The one departure: the sort is asked to be stable, which the reference's CPU sort is
    anyway - tied values (particles that were resampled and not jittered) then accumulate their weights in one defined order
    on every device, the order ``pf_jitter_fit`` uses."""
    sort, sort_indices = x.sort(dim=0, stable=True)
    cumulative_weights = w[sort_indices].cumsum(0)

    low_indices = (cumulative_weights - 0.25).abs().argmin(0)
    high_indices = (cumulative_weights - 0.75).abs().argmin(0)

    iqr = (sort[high_indices].diag() - sort[low_indices].diag()) / 1.349
    iqr2 = iqr ** 2

    w = w.unsqueeze(-1)
    if mean is None:
        mean = (w * x).sum(0)
    var = (w * (x - mean) ** 2).sum(0)

    mask = iqr2 <= var
    if mask.any():
        var[mask] = iqr2[mask]
    return var


class JitterKernel:
    """Base class of the jittering kernels (``jittering.py:92-138``).  ``std_threshold``: the smallest standard deviation
    (default: the reference's ``EPS``, the square root of the machine epsilon of the parameters' dtype)."""

    KIND: Optional[int] = None  # _lib.JITTER_*: the family as pf_jitter_fit / pf_jitter_apply know it (None: torch route only)

    def __init__(self, std_threshold: Optional[float] = None):
        self._min_std = std_threshold
        self.last_fit = None  # (mean, scale, std) of the latest torch-route ``jitter`` (the parity tests read it)

    def min_std(self, dtype) -> float:
        return _eps_of(dtype) if self._min_std is None else float(self._min_std)

    def native(self, dtype) -> Optional[Tuple[int, float, Optional[torch.Tensor]]]:
        """``(kind, par, per-parameter scale)`` for the HIP kernels - only for the family's own ``fit`` (a subclass that
        overrides it runs on the torch route)."""
        return None

    def _own_fit(self, cls) -> bool:
        return type(self).fit is cls.fit and type(self).jitter is JitterKernel.jitter

    def fit(self, x: torch.Tensor, w: torch.Tensor, indices: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        raise NotImplementedError()

    def jitter(self, x: torch.Tensor, w: torch.Tensor, indices: torch.Tensor, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``mean + std * eps`` (``jittering.py:119-133`` with ``_jitter``, :14-26); ``eps``: the standard normals (default: drawn
        from torch's global generator, like the reference)."""
        if indices.shape[0] != x.shape[0]:
            raise Exception(f"Shape of ``indices`` is not congruent with ``x``: {indices.shape[0]} != {x.shape[0]}")
        mean, scale = self.fit(x, w, indices)
        std = scale.clamp(self.min_std(x.dtype), INFTY)
        self.last_fit = (mean, scale, std)
        if eps is None:
            eps = torch.empty_like(mean).normal_()
        return mean + std * eps

    def get_ess(self, w: torch.Tensor) -> torch.Tensor:
        return w.pow(2.0).sum(dim=0).reciprocal()

    def _bw_fac(self, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        eps = _eps_of(x.dtype)
        return (1.59 * self.get_ess(w) ** (-1 / 3)).clamp(eps, 1 - eps)


class ShrinkingKernel(JitterKernel):
    """The shrinking kernel of Flury & Shephard (``jittering.py:141-160``)."""

    KIND = _lib.JITTER_SHRINKING

    def native(self, dtype):
        return (self.KIND, 0.0, None) if self._own_fit(ShrinkingKernel) else None

    def fit(self, x, w, indices):
        bw_fac = self._bw_fac(x, w)
        mean = (w.unsqueeze(-1) * x).sum(0)
        var = robust_var(x, w, mean)
        beta = math.sqrt(1.0 - bw_fac ** 2)
        means = (mean + beta * (x - mean))[indices]
        return means, bw_fac * var.sqrt()


class NonShrinkingKernel(ShrinkingKernel):
    """The non-shrinking version (``jittering.py:163-175``) - the default."""

    KIND = _lib.JITTER_NONSHRINKING

    def native(self, dtype):
        return (self.KIND, 0.0, None) if self._own_fit(NonShrinkingKernel) else None

    def fit(self, x, w, indices):
        bw_fac = self._bw_fac(x, w)
        var = robust_var(x, w)
        values = x[indices]
        return values, bw_fac * var.sqrt()


class LiuWestShrinkage(ShrinkingKernel):
    """Liu & West's shrinkage kernel (``jittering.py:178-206``)."""

    KIND = _lib.JITTER_LIUWEST

    def __init__(self, a: float = 0.98):
        super().__init__()
        self._a = a
        self._bw_fac = math.sqrt(1 - a ** 2)

    def native(self, dtype):
        return (self.KIND, float(self._a), None) if self._own_fit(LiuWestShrinkage) and 0.0 <= self._a <= 1.0 else None

    def fit(self, x, w, indices):
        mean = (w.unsqueeze(-1) * x).sum(0)
        var = robust_var(x, w, mean)
        values = (x * self._a + (1 - self._a) * mean)[indices]
        return values, self._bw_fac * var.sqrt()


class ConstantKernel(ShrinkingKernel):
    """Constant scale, as in the NESS paper (``jittering.py:209-225``).  ``scale``: a number or a tensor - one value, or one
    per parameter (the reference takes tensors only: it calls ``.clamp`` on it)."""

    KIND = _lib.JITTER_CONSTANT

    def __init__(self, scale: Union[float, torch.Tensor]):
        super().__init__()
        self._scale = scale

    def native(self, dtype):
        if not self._own_fit(ConstantKernel):
            return None
        s = self._scale
        if isinstance(s, torch.Tensor) and s.numel() > 1:
            return (self.KIND, 0.0, s.reshape(-1))
        return (self.KIND, float(s), None)

    def fit(self, x, w, indices):
        values = x[indices]
        return values, torch.as_tensor(self._scale, dtype=x.dtype, device=x.device)


class OnlineKernel:
    """The update of the online algorithms (``online.py:8-51``): resample the theta-particles, jitter them, gather the
    filters' latest state by ancestor, zero the theta-weights.  ``discrete``: only a Bernoulli(B^-1/2) share of the particles
    moves.  ``trace`` (set to a list): every update's ancestors, fit and jittered values."""

    def __init__(self, kernel: Optional[JitterKernel] = None, discrete: bool = False, resampling=theta_systematic, seed: int = 0):
        self._kernel = kernel or NonShrinkingKernel()
        self._disc = discrete
        self._resampler = resampling
        self._seed = seed
        self.updates = 0  # (also the Philox counter of the kernel route: draws are a function of (seed, update, particle, parameter))
        self.trace = None
        self.last_route = None

    def _native(self, theta: ThetaParticles, w: torch.Tensor):
        """What the kernel route needs - or None: the torch route."""
        if not (HINTS.theta_kernels and w.is_cuda and w.dim() == 1 and w.is_contiguous() and w.dtype == theta.dtype
                and w.shape[0] <= _lib.JITTER_MAXB and self._resampler is theta_systematic):
            return None
        priors = theta.native_priors()
        family = self._kernel.native(theta.dtype)
        return None if priors is None or family is None else (priors, family)

    def update(self, theta: ThetaParticles, filter_, state: SMC2State, generator=None) -> SMC2State:
        draws = generator if isinstance(generator, ThetaDraws) else NessDraws(generator) if generator is not None else None
        u = draws.uniform(()) if draws is not None else torch.rand(())
        w = state.w
        b = w.shape[0]
        stacked = theta.stack_parameters(constrained=False)
        native = self._native(theta, w)
        if native is not None:
            from .. import ops

            priors, (kind, par, scale) = native
            eps_d = _eps_of(theta.dtype)
            clamp = (eps_d, 1 - eps_d)
            indices = ops.theta_resample(w, float(u))
            fit, mean, scale_out = ops.jitter_fit(stacked, w, kind, par, scale, self._kernel.min_std(theta.dtype), clamp)
            eps = select = None
            if draws is not None and getattr(draws, "taped", False):
                eps = _to_device(draws.normal(stacked.shape), stacked)
                if self._disc:
                    select = _to_device(draws.bernoulli((b,), 1 / b ** 0.5), stacked)
            jittered = ops.jitter_apply(priors, stacked, indices, fit, kind, par, [theta[n] for n in theta.names()], self._disc,
                                        eps, select, self._seed, self.updates, clamp)
            theta.adopt_jittered(jittered)
            state.filter_state.resample(indices, entire_history=False)
            if self.trace is not None:
                self.trace.append(dict(kind="jitter", route="kernels", indices=indices, scale=fit[1].clone(), std=fit[2].clone(),
                                       weighted_mean=fit[0].clone(), ess=fit[3].clone(), jittered=jittered))
        else:
            weights = theta_normalize(w)
            indices = self._resampler(weights, u)
            eps = None
            if draws is not None:
                eps = _to_device(draws.normal(stacked.shape), stacked)
            jittered = self._kernel.jitter(stacked, weights, indices, eps)
            theta.resample(indices)
            state.filter_state.resample(indices, entire_history=False)
            if self._disc:
                if draws is not None:
                    to_jitter = _to_device(draws.bernoulli((b,), 1 / b ** 0.5), stacked).unsqueeze(-1)
                else:
                    to_jitter = torch.empty(b, device=jittered.device, dtype=jittered.dtype).bernoulli_(1 / b ** 0.5).unsqueeze(-1)
                jittered = (1 - to_jitter) * stacked[indices] + to_jitter * jittered
            theta.unstack_parameters(jittered, constrained=False)
            if self.trace is not None:
                mean, scale, std = self._kernel.last_fit
                self.trace.append(dict(kind="jitter", route="torch", indices=indices, mean=mean, scale=scale, std=std, jittered=jittered))
        self.last_route = "kernels" if native is not None else "torch"
        filter_.initialize_model(theta)
        state.w.fill_(0.0)
        self.updates += 1
        return state


class BaseOnlineAlgorithm:
    """``BaseOnlineAlgorithm`` (``ness.py:14-58``): ``filter_`` is built with a model *builder* ``theta -> StateSpaceModel``,
    ``priors`` maps parameter names to distributions (the reference's context), as for ``SMC2``.  One GPU."""

    def __init__(self, filter_, particles: int, priors, kernel: Optional[JitterKernel] = None, discrete: bool = False,
                 device="cuda", dtype=torch.float32, seed: int = 0, group=None):
        if group is not None:
            raise NotImplementedError("NESS runs on one GPU: theta-particles sharded over a process group (`group=`) are not "
                                      "supported - use SMC2 for a sharded run")
        self.filter = filter_
        self.shard = None
        self.particles = torch.Size([particles])
        self.theta = ThetaParticles(priors, particles, device, dtype)
        self.filter.set_batch_shape(self.particles)
        self._kernel = OnlineKernel(kernel=kernel or NonShrinkingKernel(), discrete=discrete, seed=seed)
        self._gen = NessDraws(torch.Generator().manual_seed(seed))
        self._seed = seed

    def initialize(self, theta0: Optional[torch.Tensor] = None) -> SMC2State:
        """Draws the theta-particles from their priors (``sequential/base.py:52-62``) - or starts from ``theta0``, their
        ``(B, P)`` stacked constrained values."""
        g = torch.Generator().manual_seed(self._seed * 7919 + 13)
        self.theta.initialize_parameters(g)
        if theta0 is not None:
            self.theta.unstack_parameters(theta0.to(device=self.theta.device, dtype=self.theta.dtype), constrained=True)
        self.filter.initialize_model(self.theta)
        init_state = self.filter.initialize()
        ll = init_state.get_loglikelihood()
        return SMC2State(torch.zeros(self.particles[0], device=ll.device, dtype=ll.dtype), self.filter.initialize_with_result(init_state))

    def _previous(self, state: SMC2State) -> Tuple[float, bool]:
        """(ESS, every weight finite) of the theta-weights after the PREVIOUS observation as host numbers: what the move left
        in the host slot - or, for a fresh / loaded state, one small copy."""
        pair = state.__dict__.get("_host_pair")
        if pair is None:
            if getattr(state, "stats", None) is None:
                state._ess()
            pair = state._host_pair = tuple(state.stats.tolist())
        return pair[0], bool(pair[1])

    def do_update_particles(self, state: SMC2State) -> bool:
        raise NotImplementedError()

    def step(self, y: torch.Tensor, state: SMC2State) -> SMC2State:
        state = self._step(y, state)
        state.current_iteration += 1
        return state

    def _step(self, y: torch.Tensor, state: SMC2State) -> SMC2State:
        """One observation (``ness.py:50-58``): the update test on the weights the PREVIOUS observation left, the update, the
        filters' move, ``w += ll_t`` - the move on the same fast path as ``SMC2.step`` (``online_move``)."""
        if self.do_update_particles(state):
            state = self._kernel.update(self.theta, self.filter, state, generator=self._gen)
        state._host_pair = online_move(self, y, state)
        return state

    def fit(self, y: torch.Tensor) -> SMC2State:
        """All observations of ``y``, one by one (the algorithm is online: there is nothing to run ahead of)."""
        state = self.initialize()
        for t in range(y.shape[0]):
            state = self.step(y[t], state)
        return state

    def posterior_mean(self, state: SMC2State) -> torch.Tensor:
        """Weighted mean of the stacked (constrained) parameters over the theta-particles."""
        return theta_normalize(state.w) @ self.theta.stack_parameters(True)

    def forecast(self, state: SMC2State, steps: int, seed: Optional[int] = None, route: str = "auto", covariance: bool = False):
        """The posterior predictive ``steps`` moves ahead: the filters' forecasts mixed with the normalised theta-weights
        (``smc2.posterior_forecast``)."""
        return posterior_forecast(self.filter, state, steps, seed, None, route, covariance)


class NESS(BaseOnlineAlgorithm):
    """``NESS(filter_, particles, threshold=0.9, kernel=None, discrete=False)`` (``ness.py:61-85``): the update fires when the
    ESS of the theta-weights is below ``threshold * particles`` or a weight is not finite."""

    def __init__(self, filter_, particles: int, priors, threshold: float = 0.9, **kwargs):
        super().__init__(filter_, particles, priors, **kwargs)
        self._threshold = threshold * particles

    def do_update_particles(self, state: SMC2State) -> bool:
        ess, finite = self._previous(state)
        return ess < self._threshold or not finite


class FixedWidthNESS(BaseOnlineAlgorithm):
    """The fixed observation width version (``ness.py:88-111``): an update every ``block_len`` calls, or when a weight is not
    finite."""

    def __init__(self, filter_, particles: int, priors, block_len: int = 125, **kwargs):
        super().__init__(filter_, particles, priors, **kwargs)
        self._bl = block_len
        self._num_iterations = 0

    def do_update_particles(self, state: SMC2State) -> bool:
        self._num_iterations += 1
        _, finite = self._previous(state)
        return (self._num_iterations % self._bl == 0) or not finite
