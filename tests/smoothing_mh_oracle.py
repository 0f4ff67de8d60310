"""TEST INFRASTRUCTURE - host oracle, cases and bars of the ``"ffbs-mh"`` tests (``tests/test_smoothing_mh_oracle_cpu.py``,
``tests/test_smoothing_mh_gpu.py``): backward simulation by Metropolis-Hastings (Bunch & Godsill 2013) as ``pf_smooth_mh`` states
it (``include/pf_amd.h``, ``csrc/pf_smooth_mh.hpp``), restated with torch on the CPU.

Per filter column b and trajectory j, for t = S - 2 .. 0 with x+ = out[t + 1][j] and k+ = idx_out[t + 1][b][j]:

* start: i = anc[t + 1][k+], l = l_t(i), or -inf when candidate i's sanitised log-weight is -inf;
* K rounds with uniforms (u1, u2): the proposal i' is the first candidate with cdf_t[i'] > u1 cdf_t[N - 1] - none: the last
  candidate of positive mass (``cpu_ref.ffbs_backward_step``'s convention) -, cdf_t the inclusive running sum in float64 of
  exp(sanitised logw_t - max), max and exp in the computing dtype; accepted iff l = -inf or log(u2) < l_t(i') - l in that dtype;
* pick = i.

l_t(i) is ``oracle.models.transition_log_prob`` of x+ under ``oracle.models.mean_scale`` of candidate i: the kernel's l plus a
constant of the filter (log sqrt(2 pi)), which no difference l' - l sees.  The matrix kind's model is ``tests/linmat_oracle.py``'s
rows through ``linmat_smoothing_cases.spec_of_rows``.

A step is teacher-forced with ``(out[t + 1], idx_out[t + 1])`` where given, so one differing pick cannot move the later ones.  Per
chain the oracle returns the pick and two margins: the smallest distance of u1 to a boundary of the normalised cdf over the rounds
and the smallest ``|log u2 - (l' - l)|`` - a kernel that picks otherwise than the float64 oracle must have one of them small."""
import functools
import math

import torch

from oracle import cpu_ref
from oracle import models as M
from tests import linmat_smoothing_cases as lsc
from tests import smoothing_cases as sc

F64_ACCEPT_BAR = 1e-9  # relative to max(1, |l|, |l'|): the float64 bar of the README's parity table
INF = math.inf


class Case:
    """A ``smoothing_cases.History`` (built-in kind or matrix kind) with ancestors ``anc (S, N, B)`` int64 (row 0 is never read),
    the resampled indices of the last state ``idx_last (N, B)`` int64, ``k`` rounds and their tape ``u (S - 1, K, 2, N, B)`` in the
    history's dtype."""

    def __init__(self, h, anc, idx_last, k, u):
        self.h, self.anc, self.idx_last, self.k, self.u = h, anc, idx_last, k, u
        assert anc.shape == (h.s, h.n, h.b) and idx_last.shape == (h.n, h.b) and u.shape == (max(h.s - 1, 0), k, 2, h.n, h.b)

    def edited(self, **kw):
        f = dict(h=self.h, anc=self.anc, idx_last=self.idx_last, k=self.k, u=self.u)
        f.update(kw)
        return Case(**f)

    def device_inputs(self, device="cuda"):
        """The library's layouts: ``x_hist (S, D, B, N)``, ``logw_hist (S, B, N)``, ``anc_hist (S, B, N)`` int32, ``idx_last (B, N)``
        int32, ``u (S - 1, K, 2, B, N)``."""
        x_hist, logw, _, _ = self.h.soa(device)
        anc = self.anc.permute(0, 2, 1).contiguous().to(torch.int32).to(device)
        idx_last = self.idx_last.t().contiguous().to(torch.int32).to(device)
        u = self.u.permute(0, 1, 2, 4, 3).contiguous().to(device)
        return x_hist, logw, anc, idx_last, u


def _draws(h, k, seed):
    gen = torch.Generator().manual_seed(12000 + seed)
    anc = torch.randint(h.n, (h.s, h.n, h.b), generator=gen)
    idx_last = torch.randint(h.n, (h.n, h.b), generator=gen)
    u = torch.rand((max(h.s - 1, 0), k, 2, h.n, h.b), generator=gen, dtype=torch.float64).to(h.dtype)
    return anc, idx_last, u


@functools.lru_cache(maxsize=None)
def case(model, n, b, s, dtype, k, seed=0):
    """``smoothing_cases.synthetic`` (``model`` a name) or ``linmat_smoothing_cases.synthetic`` (``model`` a dimension) with seeded
    random ancestors, last indices and uniforms."""
    h = lsc.synthetic(model, n, b, s, dtype, seed) if isinstance(model, int) else sc.synthetic(model, n, b, s, dtype, seed)
    anc, idx_last, u = _draws(h, k, seed)
    return Case(h, anc, idx_last, k, u)


def edge_case(model, n, b, s, dtype, k, seed=1):
    """The same on ``edge_history``'s weights (a NaN, a +inf and the lowest finite value on candidates 0, 1, 2 of column 0 of
    state 0; all of column 1's mass on candidate N - 1; no mass on candidates 256 .. 511 of state 1)."""
    h = lsc.edge_history(model, n, b, s, dtype, seed) if isinstance(model, int) else sc.edge_history(model, n, b, s, dtype, seed)
    anc, idx_last, u = _draws(h, k, seed)
    return Case(h, anc, idx_last, k, u)


TRAILING_DEAD = 100  # candidates without mass behind the last live one in ``fallback_case``


def fallback_case(model, n, b, s, dtype, k, seed=1):
    """A ``case`` whose last ``TRAILING_DEAD`` candidates of every state carry no mass - the last candidate of positive mass is
    ``N - 1 - TRAILING_DEAD``, not ``N - 1`` - with ``u2 = 0`` (accept) everywhere and, for chains 0 .. 9, ``u1 = 1`` in every
    round: ``u1 x total`` IS the total, no cdf entry lies beyond it, and the proposal comes from the fallback.  (A tape value
    below 1 does not get there in general: in float32 ``(1 - 2^-24) x total`` in double is below the total, and in float64
    ``(1 - 2^-53) x total`` rounds to the total's predecessor unless the total is a power of two.)"""
    base = case(model, n, b, s, dtype, k, seed)
    logw = [w.clone() for w in base.h.logw]
    for w in logw:
        w[n - TRAILING_DEAD:] = -INF
    u = base.u.clone()
    u[:, :, 1] = 0.0
    u[:, :, 0, :10] = 1.0
    return base.edited(h=base.h.edited(logw=logw), u=u)


def label(model, n, b, s, k):
    return f"{'linmat-D%d' % model if isinstance(model, int) else model} {n}x{b}x{s} K={k}"


# the cases of the parity sweeps: (model name or matrix dimension, N, B, S, K) - every model at two shapes, sine and lorenz at every
# shape of ``smoothing_cases.SHAPES``, K in {0, 1} for sine, the matrix kind at ``linmat_smoothing_cases.DIMS``
DRAW_CASES = tuple([(m,) + s + (4,) for m in sc.MODELS for s in sc.EVERY_MODEL_AT]
                   + [(m,) + s + (4,) for m in sc.EVERY_SHAPE_WITH for s in sc.SHAPES if s not in sc.EVERY_MODEL_AT]
                   + [("sine",) + s + (k,) for s in sc.EVERY_MODEL_AT for k in (0, 1)]
                   + [(d,) + s + (4,) for d in lsc.DIMS for s in sc.EVERY_MODEL_AT])
DRAW_IDS = [label(*c).replace(" ", "-") for c in DRAW_CASES]


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def sanitised(h, t, dtype):
    """Log-weights of state t as a backward draw takes them (sanitised in the dtype they are held in), in ``dtype``."""
    return cpu_ref.ffbs_sanitize_logw(h.logw[t]).to(dtype)


def cdf_of(h, t, dtype):
    """``(cdf (N, B) float64, last_pos (B,))``: the inclusive running sum of exp(sanitised logw_t - max), max and exp in ``dtype``;
    the last candidate of positive mass (N - 1 where there is none)."""
    w = sanitised(h, t, dtype)
    m = w.max(dim=0, keepdim=True)[0]
    e = torch.where(w == -INF, torch.zeros_like(w), (w - m).exp()).double()
    cdf = e.cumsum(dim=0)
    last_pos = (h.n - 1) - (e > 0).flip(0).to(torch.int64).argmax(dim=0)
    return cdf, last_pos


def ell(h, spec, t, dtype, x_next, idx):
    """l_t(idx) ``(N, B)`` in ``dtype``: the transition log-density of ``x_next (N, B, [D])`` given candidates ``idx (N, B)`` of state t."""
    xi = sc.gather(h.x[t].to(dtype), idx)
    loc, scale = M.mean_scale(spec, xi)
    return M.transition_log_prob(spec, x_next.to(dtype), loc, scale)


def step(c, dtype, t, x_next, k_next):
    """One backward step for every chain, computing in ``dtype``, from ``x_next (N, B, [D])`` (values of ``h.dtype``) at the
    indices ``k_next (N, B)`` of state t + 1.  Returns ``pick (N, B)``, the margins ``margin_p``, ``margin_a`` (absolute) and
    ``margin_a_rel`` (relative to max(1, |l|, |l'|)) ``(N, B)`` float64 - inf where no round could have gone the other way -, the
    normalised cdf ``cdf_norm (N, B)`` and per round ``cur``, ``prop`` ``(K, N, B)``, ``dl (K, N, B)`` float64 and ``fallback (K, N, B)``
    bool: no candidate lay beyond the target and the proposal is the last candidate of positive mass."""
    h = c.h
    spec = h.spec(dtype)
    n, b = h.n, h.b
    cdf, last_pos = cdf_of(h, t, dtype)
    total = cdf[-1]  # (B,)
    cdf_norm = cdf / total
    i = c.anc[t + 1].gather(0, k_next)
    dead = sanitised(h, t, dtype).gather(0, i) == -INF
    l = torch.where(dead, torch.full((n, b), -INF, dtype=dtype), ell(h, spec, t, dtype, x_next, i))
    big = torch.full((n, b), INF, dtype=torch.float64)
    margin_p, margin_a, margin_a_rel = big.clone(), big.clone(), big.clone()
    cur, prop, dl, fell = [], [], [], []
    for r in range(c.k):
        u1, u2 = c.u[t, r, 0].to(dtype), c.u[t, r, 1].to(dtype)
        target = u1.double() * total
        ip = torch.searchsorted(cdf.t().contiguous(), target.t().contiguous(), right=True).t()  # first candidate with cdf > target
        fell.append(ip >= n)  # no candidate beyond the target: the fallback
        ip = torch.where(ip >= n, last_pos.expand(n, b), ip)
        below = torch.where(ip > 0, cdf_norm.gather(0, (ip - 1).clamp(min=0)), torch.zeros_like(target))
        dist = torch.minimum((u1.double() - cdf_norm.gather(0, ip)).abs(), (u1.double() - below).abs())
        margin_p = torch.minimum(margin_p, torch.nan_to_num(dist, nan=INF))
        lp = ell(h, spec, t, dtype, x_next, ip)
        d = lp - l
        accept = (l == -INF) | (torch.log(u2) < d)
        gap = (torch.log(u2).double() - d.double()).abs()
        gap = torch.where((l == -INF) | gap.isnan(), big, gap)
        margin_a = torch.minimum(margin_a, gap)
        margin_a_rel = torch.minimum(margin_a_rel, gap / torch.maximum(torch.ones_like(gap), torch.maximum(l.double().abs(), lp.double().abs())))
        cur.append(i), prop.append(ip), dl.append(d.double())
        i, l = torch.where(accept, ip, i), torch.where(accept, lp, l)
    stack = lambda v, dt: torch.stack(v, 0) if v else torch.empty((0, n, b), dtype=dt)  # noqa: E731
    return dict(pick=i, margin_p=margin_p, margin_a=margin_a, margin_a_rel=margin_a_rel, cdf_norm=cdf_norm, cur=stack(cur, torch.int64),
                prop=stack(prop, torch.int64), dl=stack(dl, torch.float64), fallback=stack(fell, torch.bool))


def oracle_pass(c, dtype, forced=None):
    """The backward pass over ``c`` computing in ``dtype``: the ``step`` results as a list indexed by t = 0 .. S - 2.  ``forced(t + 1)
    -> (x_next (N, B, [D]), k_next (N, B))`` teacher-forces a step; else the pass follows its own picks from ``idx_last``."""
    h = c.h
    res = [None] * (h.s - 1)
    k_next = c.idx_last
    for t in range(h.s - 2, -1, -1):
        if forced is not None:
            x_next, k_next = forced(t + 1)
        else:
            x_next = sc.gather(h.x[t + 1], k_next)
        res[t] = step(c, dtype, t, x_next, k_next)
        k_next = res[t]["pick"]
    return res


def paths_of(c, ref):
    """``(out (S, N, B, [D]), idx (S, N, B))`` of a free-running ``oracle_pass``."""
    idx = [r["pick"] for r in ref] + [c.idx_last]
    return torch.stack([sc.gather(c.h.x[t], idx[t]) for t in range(c.h.s)], 0), torch.stack(idx, 0)


# ---- the bars -------------------------------------------------------------------------------------------------------------
def deltas(c, ref64, ref32=None):
    """``(delta_p, delta_a)``.  float64 histories: ``sc.f64_delta(N)`` - a parallel scan adds in another order - and ``None``:
    the acceptance bar is ``F64_ACCEPT_BAR`` relative to max(1, |l|, |l'|).  float32 histories: 4 x the float32 oracle's own error
    against the float64 oracle on the case (``ref32``: its pass under the same teacher) - of the normalised cdf, and of l' - l in
    the rounds both oracles made with the same pair of candidates."""
    if c.h.dtype == torch.float64:
        return sc.f64_delta(c.h.n), None
    dp, da = 0.0, 0.0
    for a, b in zip(ref32, ref64):
        dp = max(dp, float((a["cdf_norm"] - b["cdf_norm"]).abs().nan_to_num(nan=0.0).max()))
        same = (a["cur"] == b["cur"]) & (a["prop"] == b["prop"]) & a["dl"].isfinite() & b["dl"].isfinite()
        if bool(same.any()):
            da = max(da, float((a["dl"] - b["dl"])[same].abs().max()))
    return 4.0 * dp, 4.0 * da


def compare(c, idx, ref, delta_p, delta_a, what):
    """``idx (S, N, B)`` against the float64 oracle's teacher-forced steps ``ref``: a chain whose pick differs has a boundary margin
    <= ``delta_p`` or an acceptance margin <= ``delta_a`` (``None``: the relative float64 bar), and at most ``sc.MAX_DISAGREE`` of
    the case's chains differ.  Returns ``(differing chains, chains, their largest boundary margin, their largest acceptance margin)``."""
    h = c.h
    bad, total, worst_p, worst_a = 0, 0, 0.0, 0.0
    assert torch.equal(idx[-1], c.idx_last), f"{what}: the last state's indices are not idx_last"
    for t in range(h.s - 1):
        assert bool((idx[t] >= 0).all()) and bool((idx[t] < h.n).all()), f"{what}: state {t} names a particle outside the column"
        total += idx[t].numel()
        r = ref[t]
        for j, b in (idx[t] != r["pick"]).nonzero().tolist():
            mp = float(r["margin_p"][j, b])
            ma = float(r["margin_a"][j, b]) if delta_a is not None else float(r["margin_a_rel"][j, b])
            bar_a = delta_a if delta_a is not None else F64_ACCEPT_BAR
            bad += 1
            assert mp <= delta_p or ma <= bar_a, (
                f"{what}: state {t} chain {j} column {b} picked {int(idx[t][j, b])}, the oracle {int(r['pick'][j, b])}: boundary margin "
                f"{mp:.3e} (allowed {delta_p:.3e}), acceptance margin {ma:.3e} (allowed {bar_a:.3e})")
            if mp <= delta_p:
                worst_p = max(worst_p, mp)
            else:
                worst_a = max(worst_a, ma)
    assert bad <= sc.MAX_DISAGREE * total, f"{what}: {bad} of {total} chains differ from the float64 oracle"
    return bad, total, worst_p, worst_a


# ---- the law the chain targets ------------------------------------------------------------------------------------------------
LIVE, CHI2_BAR = 16, 60.0


def law_case(model, dtype, k, n=4096, seed=2):
    """N chains from ONE x+, only candidates 0 .. 15 of state 0 alive, random - mostly dead - starts: state 1 holds one value N
    times, ``idx_last`` is the identity and ``anc[1]`` is random, so chain j starts at ``anc[1][j]`` and all chains target the same
    categorical: p_i ~ W_i p(x+ | x_0^i) over the live candidates."""
    base = sc.synthetic(model, n, 1, 2, dtype, seed)
    logw0 = base.logw[0].clone()
    logw0[LIVE:] = -INF
    x1 = base.x_last[:1].expand_as(base.x_last).contiguous()
    h = sc.History(model, dtype, [base.x[0], x1], [logw0, base.logw[1]], x1, base.u)
    gen = torch.Generator().manual_seed(13000 + seed)
    anc = torch.randint(n, (2, n, 1), generator=gen)
    u = torch.rand((1, k, 2, n, 1), generator=gen, dtype=torch.float64).to(dtype)
    return Case(h, anc, torch.arange(n).unsqueeze(-1), k, u)


def law_chi2(c, picks):
    """Chi-square of ``picks (N,)`` against the backward categorical of the float64 oracle (``cpu_ref.ffbs_backward_step``) over the
    live candidates with an expected count >= 5; no pick may be a dead candidate.  Returns ``(chi2, bins)``."""
    h = c.h
    spec = h.spec(torch.float64)
    w = cpu_ref.ffbs_sanitize_logw(h.logw[0]).double()
    _, cdf = cpu_ref.ffbs_backward_step(spec, h.x[0].double(), w, h.x[1][:1].double(), torch.zeros(1, 1, dtype=torch.float64))
    p = torch.diff(cdf[0, 0], prepend=torch.zeros(1, dtype=torch.float64))
    assert bool((picks < LIVE).all()) and bool((picks >= 0).all()), "a candidate without mass was picked"
    obs = torch.bincount(picks, minlength=h.n).double()
    expected = picks.numel() * p
    use = expected >= 5.0
    return float(((obs[use] - expected[use]) ** 2 / expected[use]).sum()), int(use.sum())


# ---- the kernel's own draws ---------------------------------------------------------------------------------------------------
PHILOX_STREAM = 10


def philox_uniforms(seed, s, k, n, b, dtype):
    """The tape ``(S - 1, K, 2, N, B)`` a NULL-tape call draws: one Philox call per round, call number ``(b N + j) K + r`` of
    ``(seed, stream 10, step t)``, slot 0 proposes and slot 1 accepts (``philox_ref.call`` / ``_slot_values`` with ``u01`` / ``u01_d``)."""
    import numpy as np

    from tests import philox_ref as P

    u = torch.empty((max(s - 1, 0), k, 2, n, b), dtype=torch.float64)
    j, col = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(b, dtype=np.uint64), indexing="ij")  # (N, B)
    for t in range(s - 1):
        for r in range(k):
            counter = (col * np.uint64(n) + j) * np.uint64(k) + np.uint64(r)
            slots = P._slot_values(P.call(seed, PHILOX_STREAM, t, counter), dtype, P.u01, P.u01_d)
            u[t, r, 0], u[t, r, 1] = torch.from_numpy(slots[0]), torch.from_numpy(slots[1])
    return u.to(dtype)
