"""Nested proposal of Naesseth et al. (``proposals/nested.py:8-50``): per particle ``num_samples`` candidates from the transition,
weighed with ``p(y | candidate)``; one is kept with probability proportional to that weight and the particle's importance weight
is ``log mean_j p(y | candidate_j)``.  It uses ``y_t`` when it draws ``x_t`` for ANY observation density - the stochastic
volatility model has no other proposal that does - and needs no gradients.

* a built-in model of up to three state / observation components: ``pf_nested_sample_and_weight`` (``csrc/pf_nested.hpp``), one
  launch, nothing ``num_samples``-fold in memory;
* anything else (user callables, ``LinearModel``, more than ``PF_NESTED_MAX`` candidates, a custom ``pre_weight_func``,
  ``HINTS.nested_kernel = False``): the same sequence as PyTorch-ROCm operations.

Two intentional differences from the reference on both routes: the weight is evaluated in its max-shifted form
(the reference's ``log_prob.exp().mean(0).log()`` is ``-inf`` once every candidate's density underflows ``exp``; the two agree
wherever the reference's is finite), and the pick is the inverse CDF of ONE uniform per particle (the law of the reference's
``Categorical.sample``, from an injectable draw).  The filter runs step by step: the fused kernels know two proposals."""
import math
from typing import Optional

import torch
from torch.distributions import Independent, Normal

from .... import _lib as L
from .... import ops
from ....hints import HINTS
from ....timeseries import AffineProcess, TimeseriesState
from .base import Proposal


class NestedProposal(Proposal):
    """``record_picks`` / ``last_pick`` exist for the tests: with ``record_picks = True`` a move leaves the index of the candidate
    it kept in ``last_pick (N, [B])`` (the kernel then writes its optional ``pick_out``)."""

    # The torch route evaluates at most this many candidates at once (it walks the particles in slices): its tensors are
    # ``num_samples``-fold, and a linear observation of a vector state is a batched matmul with one batch entry per candidate.
    # 2^22 is a size this route has been run at; a single call over 2^26 candidates of a 3-component state ended in a device memory
    # fault inside the torch operations (profiles/nested_proposal.txt) - which operation's limit that was is not established.
    TORCH_CANDIDATES = 1 << 22

    def __init__(self, num_samples: int, **kwargs):
        super().__init__(**kwargs)
        if int(num_samples) != num_samples or int(num_samples) < 1:
            raise ValueError(f"num_samples must be a positive integer, got {num_samples!r}")
        self._num_samples = int(num_samples)
        self._z_tape: Optional[torch.Tensor] = None
        self._v_tape: Optional[torch.Tensor] = None
        self.record_picks = False
        self.last_pick: Optional[torch.Tensor] = None

    @property
    def num_samples(self) -> int:
        return self._num_samples

    def set_tape(self, z: Optional[torch.Tensor] = None, v: Optional[torch.Tensor] = None):
        """Parity mode: the candidates' standard normals ``z (T, M, N, [B], [D])`` (row ``z[t, 0]`` is the transition's draw of a
        propagate-only move) and the picks' uniforms ``v (T, N, [B])``, in the reference's layout.  The filter's own
        ``set_tape(u=, z0=)`` supplies the resampling offsets and the initial draw."""
        self._z_tape, self._v_tape = z, v
        return self

    @property
    def uses_kernels(self) -> bool:
        c = self._ctx
        return (c is not None and HINTS.nested_kernel and not self._custom_pre_weight and not c.kind.is_user
                and c.kind.hid_kind != L.HID_LINEAR_MAT and c.kind.dim <= L.MAX_D and c.kind.obs_dim <= L.MAX_O
                and self._num_samples <= L.NESTED_MAX)

    # -- tapes ---------------------------------------------------------------------------------------------------------
    def _z_at(self, step: int, like: torch.Tensor) -> Optional[torch.Tensor]:
        return None if self._z_tape is None else self._z_tape[step].to(device=like.device, dtype=like.dtype)

    def _v_at(self, step: int, like: torch.Tensor) -> Optional[torch.Tensor]:
        return None if self._v_tape is None else self._v_tape[step].to(device=like.device, dtype=like.dtype)

    @staticmethod
    def _candidates_soa(z: torch.Tensor, batched: bool, has_event: bool) -> torch.Tensor:
        """``(M, N, [B], [D])`` -> the kernel's ``(M, D, B, N)``."""
        if not has_event:
            z = z.unsqueeze(-1)
        if not batched:
            z = z.unsqueeze(2)
        return z.permute(0, 3, 2, 1).contiguous()

    # -- the transition alone (unobserved steps, NaN rows) ----------------------------------------------------------------
    def _propagate(self, x: TimeseriesState) -> TimeseriesState:
        step = int(x.time_index)
        z = self._z_at(step, x.value)
        if self.uses_kernels:
            c = self._ctx
            z_soa = None if z is None else ops.to_soa(z[0], c.batched, c.has_event)
            soa = ops.to_soa(x.value, c.batched, c.has_event)
            x_out, _ = ops.sample_and_weight_soa(c.kind, c.params, L.PROP_BOOTSTRAP, soa, None, z_soa, c.seed, step, weigh=False)
            return x.propagate_from(values=ops.from_soa(x_out, c.batched, c.has_event))
        if z is None:
            return self._model.hidden.propagate(x)
        return x.propagate_from(values=self._transition_draws(x, z[0]))

    def _transition_draws(self, x: TimeseriesState, z: torch.Tensor) -> torch.Tensor:
        """Draws of ``hidden.build_density(x)`` from given standard normals ``z (..., N, [B], [D])`` (parity mode, torch route)."""
        hidden = self._model.hidden
        inc = getattr(hidden, "increment_distribution", None)
        base = inc.base_dist if isinstance(inc, Independent) else inc
        if not isinstance(hidden, AffineProcess) or not isinstance(base, Normal):
            raise L.PfAmdError("a z tape needs an affine process with Gaussian increments")
        loc, scale = hidden.mean_scale(x)
        kind = getattr(self._model, "kernel_kind", None)  # (its increment scale is a host double; the distribution's may be rounded to float32)
        return loc + scale * (z * kind.inc_scale if kind is not None else base.loc + base.scale * z)

    # -- reference API ----------------------------------------------------------------------------------------------------
    def pre_weight(self, y, x):
        """The base class's ``log p(y | one-step mean)``; on a built-in model the Bootstrap branch of ``pf_pre_weight``."""
        if self.uses_kernels:
            return self._kernel_pre_weight(y, x, proposal=L.PROP_BOOTSTRAP)
        return super().pre_weight(y, x)

    def sample_and_weight(self, y, prediction):
        x = prediction.get_timeseries_state()
        step = int(x.time_index)
        m = self._num_samples
        z, v = self._z_at(step, x.value), self._v_at(step, x.value)
        if self.uses_kernels:
            c = self._ctx
            soa = ops.to_soa(x.value, c.batched, c.has_event)
            x_out, w_out, pick = ops.nested_sample_and_weight_soa(
                c.kind, c.params, m, soa, y, None if z is None else self._candidates_soa(z, c.batched, c.has_event),
                None if v is None else ops.to_cols(v), c.seed, step, want_pick=self.record_picks)
            if self.record_picks:
                self.last_pick = ops.from_cols(pick, c.batched).long()
            return x.propagate_from(values=ops.from_soa(x_out, c.batched, c.has_event)), ops.from_cols(w_out, c.batched)

        # the torch route, over slices of the particles: no operation sees more than TORCH_CANDIDATES candidates at once
        n = x.value.shape[0]
        per_particle = max(1, x.value.numel() // max(n, 1))   # state components x filters of one particle index
        rows = max(1, self.TORCH_CANDIDATES // (m * per_particle))
        parts = []
        for lo in range(0, n, rows):
            hi = min(n, lo + rows)
            parts.append(self._torch_sample_and_weight(y, x if (lo == 0 and hi == n) else x.copy(values=x.value[lo:hi]), m,
                                                       None if z is None else z[:, lo:hi], None if v is None else v[lo:hi]))
        values, weight, pick = parts[0] if len(parts) == 1 else (torch.cat([p[k] for p in parts], dim=0) for k in range(3))
        if self.record_picks:
            self.last_pick = pick
        return x.propagate_from(values=values), weight

    def _torch_sample_and_weight(self, y, x: TimeseriesState, m: int, z, v):
        """The reference's sequence (nested.py:27-47) as torch operations on the particles of ``x``: (kept candidates, weights,
        picks)."""
        if z is None:
            candidates = self._model.hidden.build_density(x).sample(torch.Size([m]))     # (M, N, [B], [D])
        else:
            candidates = self._transition_draws(x, z)
        trial = x.propagate_from(values=candidates)
        log_prob = self._model.build_density(trial).log_prob(y).nan_to_num(nan=-math.inf, posinf=-math.inf, neginf=-math.inf)
        top = log_prob.max(dim=0)[0]
        dead = top == -math.inf                                                          # no valid candidate: weight -inf, uniform pick
        mass = (log_prob - torch.where(dead, torch.zeros_like(top), top)).exp()          # (M, N, [B])
        total = mass.sum(dim=0)
        weight = torch.where(dead, top, top + (total / m).log())
        if v is None:
            v = torch.rand(top.shape, device=top.device, dtype=top.dtype)
        # the first j whose running sum exceeds v sum; should rounding leave the last running sum <= v sum, the last candidate of
        # positive mass (what the kernel keeps); no valid candidate: min(floor(v M), M - 1)
        passed = mass.cumsum(dim=0) > v * total
        first = passed.to(torch.uint8).argmax(dim=0)
        last_live = (m - 1) - (mass > 0).flip(0).to(torch.uint8).argmax(dim=0)
        pick = torch.where(passed.any(dim=0), first, last_live)
        pick = torch.where(dead, (v.double() * m).floor().long().clamp(max=m - 1), pick)
        index = pick.unsqueeze(0)
        if candidates.dim() > index.dim():
            index = index.unsqueeze(-1).expand(index.shape + candidates.shape[index.dim():])
        return candidates.gather(0, index)[0], weight, pick

    def copy(self) -> "Proposal":
        return NestedProposal(self._num_samples, pre_weight_func=self._pre_weight_func if self._custom_pre_weight else None)
