"""TEST INFRASTRUCTURE - a torch-CPU restatement of the nested proposal (``proposals/nested.py:27-47``) on explicit draw tapes,
in the role ``oracle/cpu_ref.py`` has for the other two proposals: per particle ``M`` candidates from the transition, their
observation log-densities (NaN / +inf -> -inf), one candidate kept by inverse CDF from one uniform, weight = log mean density.

The two forms this package states differently from the reference (differences) are stated here as the package
states them - equal to the reference's whenever the reference's value is finite:

* the weight in its max-shifted form ``max + log(sum exp(lp - max) / M)``;
* the pick as the first ``j`` whose running sum of ``exp(lp_j - max)`` exceeds ``v * sum`` - the last candidate of positive weight should rounding leave no such ``j`` - (the fixtures' ``Categorical`` stand-in
  counts ``cumsum(softmax) < v``: the same index but for ties of measure zero); all candidates invalid: ``min(floor(v M), M - 1)``.

``tests/test_nested_cpu.py`` pins it to the fixtures recorded from the unmodified reference (``tools/make_golden_nested.py``)."""
import math

import torch

from oracle import cpu_ref, models as M


def assert_weights_match(w, w_ref, **tol):
    """Log-weights against the reference's.  The reference's weight ``log mean exp(lp)`` is UNSHIFTED: in float64 it is -inf
    once every candidate's ``lp`` is below log(4.9e-324) = -744.4, where the shifted form is finite and <= -744.4.  Such a
    particle's accumulated SISR weight adds at most the steps' largest log-densities to that (log(1 / (s sqrt(2 pi))) <= 1.4
    per step in these cases, <= 12 steps): wherever the reference holds -inf (or the most negative float64 its
    ``normalize`` later turns a stored -inf into) the shifted value must lie below -700; every other entry is compared to the
    tolerance."""
    dead = w_ref < -1e300
    assert bool((w[dead] < -700.0).all())
    torch.testing.assert_close(w[~dead], w_ref[~dead], **tol)


def nested_sample_and_weight(spec, y, x, z, v):
    """``x (N, [B], [D])`` parents, ``z (M, N, [B], [D])`` standard normals, ``v (N, [B])`` uniforms ->
    (kept candidate ``(N, [B], [D])``, weight ``(N, [B])``, pick ``(N, [B])`` int64)."""
    m = z.shape[0]
    loc, scale = M.mean_scale(spec, x)
    cand = loc.unsqueeze(0) + scale.unsqueeze(0) * (z * spec.inc_scale)
    lp = M.obs_log_prob(spec, y, cand).nan_to_num(-math.inf, -math.inf)  # (M, N, [B])
    mx = lp.max(dim=0)[0]
    dead = mx == -math.inf
    e = (lp - torch.where(dead, torch.zeros_like(mx), mx)).exp()  # (all -inf: exp(-inf) = 0)
    total = e.sum(0)
    w = torch.where(dead, torch.full_like(mx, -math.inf), mx + (total / m).log())
    passed = e.cumsum(0) > (v * total).unsqueeze(0)
    last_live = (m - 1) - (e > 0).flip(0).to(torch.uint8).argmax(0)  # (rounding left the last running sum <= v sum)
    pick = torch.where(passed.any(0), passed.to(torch.uint8).argmax(0), last_live)
    pick = torch.where(dead, (v * m).floor().long().clamp(max=m - 1), pick)
    idx = pick.unsqueeze(0)
    if spec.dim > 0:
        idx = idx.unsqueeze(-1).expand((1,) + pick.shape + (spec.dim,))
    return cand.gather(0, idx)[0], w, pick


def batch_filter(spec, filt, m, y, x0, z_tape, u_tape, v_tape, ess_threshold):
    """SISR / APF with the nested proposal over the tapes (``z_tape (T, M, N, [B], [D])``, row 0 of a step being the
    transition's draw when its observation is NaN).  Per-step ``x, w, ll, idx, pick`` and the result's moments / total."""
    n, has_d = x0.shape[0], spec.dim > 0
    x = x0
    w = torch.zeros(x0.shape[: x0.dim() - (1 if has_d else 0)], dtype=x0.dtype)
    prev = torch.arange(n)
    if w.dim() > 1:
        prev = prev.unsqueeze(-1).expand(w.shape)
    identity = prev
    ll_total = torch.zeros(w.shape[1:], dtype=x0.dtype)
    means = [cpu_ref.get_filter_mean_and_variance(x, cpu_ref.normalize(w), has_d)[0]]
    steps = {k: [] for k in ("x", "w", "ll", "idx", "pick")}
    thr = ess_threshold * n
    for t in range(y.shape[0]):
        y_t, u = y[t], u_tape[t]
        if bool(y_t.isnan().all()):
            if filt == "sisr":
                x, w, _, idx, _ = cpu_ref.sisr_predict(spec, x, w, prev, u, thr)
            else:
                idx = identity
            x, w, ll = cpu_ref.propagate_only_step(spec, x, w, z_tape[t][0])
            pick = torch.full(w.shape, -1, dtype=torch.int64)
        elif filt == "sisr":
            x, w, W, idx, _ = cpu_ref.sisr_predict(spec, x, w, prev, u, thr)
            x, wi, pick = nested_sample_and_weight(spec, y_t, x, z_tape[t], v_tape[t])
            w = wi + w
            ll = cpu_ref.log_likelihood(wi, W)
        else:
            W_prev = cpu_ref.normalize(w)
            pre = cpu_ref.default_pre_weight(spec, y_t, x)
            idx = cpu_ref.systematic(pre + w, u=u.reshape(-1, 1))
            x, ws, pick = nested_sample_and_weight(spec, y_t, cpu_ref.batched_gather(x, idx, 0), z_tape[t], v_tape[t])
            w = ws - pre.gather(0, idx)
            ll = cpu_ref.log_likelihood(w) + (W_prev * pre.exp()).sum(dim=0).log()
        prev = idx
        means.append(cpu_ref.get_filter_mean_and_variance(x, cpu_ref.normalize(w), has_d)[0])
        ll_total = ll_total + ll
        for k, val in zip(("x", "w", "ll", "idx", "pick"), (x, w, ll, idx, pick)):
            steps[k].append(val.clone())
    out = {f"step_{k}": torch.stack(val, 0) for k, val in steps.items()}
    out["filter_means"] = torch.stack(means, 0)
    out["loglikelihood"] = ll_total
    return out
