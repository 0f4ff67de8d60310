"""TEST INFRASTRUCTURE - inputs and checks of the smoothing-kernel tests (``tests/test_smoothing_kernels_gpu.py``,
``tests/test_smoothing_oracle_cpu.py``): synthetic state histories for direct ``pf_smooth_ffbs`` / ``pf_smooth_fixed_lag`` calls and
the per-draw comparison of backward draws with the float64 oracle (``oracle.cpu_ref.ffbs_backward_step``).

Every value is generated in float64 and rounded to the dtype under test; the oracle (in float64 or in that dtype) and the kernel
start from the same rounded numbers, the model's parameters included (``rounded_spec``)."""
import functools
import math

import torch

from oracle import cpu_ref
from oracle import models as M
from oracle.cases import build_spec
from tests.nested_cases import rounded_spec

MODELS = ("lg1d", "sine", "sv_batched", "ou_batched", "rw2d", "rw2d_theta", "lorenz", "lorenz_s")
# (N, B, S): a single particle; far below one staged tile of 256 candidates; one short of / exactly / one into the second tile; a
# ragged last tile; six tiles and one particle; S = 1 (no backward draw)
SHAPES = ((1, 2, 3), (5, 1, 2), (255, 3, 3), (256, 1, 3), (257, 2, 3), (1000, 1, 4), (1537, 3, 4), (300, 2, 1))
EVERY_MODEL_AT = ((257, 2, 3), (1537, 3, 4))
EVERY_SHAPE_WITH = ("sine", "lorenz")
EDGE_CASES = (("sine", 600, 2, 3), ("rw2d", 600, 1, 3))
DRAW_CASES = tuple([(m,) + s for m in MODELS for s in EVERY_MODEL_AT]
                   + [(m,) + s for m in EVERY_SHAPE_WITH for s in SHAPES if s not in EVERY_MODEL_AT])
MIN_EFFECTIVE = 8.0  # median 1 / sum p^2 of a backward draw's categorical below which a case only checks an argmax
MAX_DISAGREE = 1e-3  # the share of a case's draws that may differ from the float64 oracle at all


def min_effective(n):
    """The input condition on a history of ``n`` particles: a median of at least 8 effective candidates per draw.  A categorical
    over ``n`` candidates has at most ``n`` of them, and log-weights of 1.5 randn alone leave about ``n / exp(1.5^2)`` = n / 9.5:
    below 128 particles the condition is that share of what ``n`` allows (``n / 16``), and never less than one candidate."""
    return min(MIN_EFFECTIVE, max(1.0, n / 16.0))


class History:
    """``x (S x (N, B, [D]))``, ``logw (S x (N, B))``, ``x_last (N, B, [D])`` and the tape ``u (S - 1, N, B)`` in ``dtype`` on the
    CPU, in the reference's layout (always batched: B may be 1)."""

    def __init__(self, model, dtype, x, logw, x_last, u):
        self.model, self.dtype = model, dtype
        self.x, self.logw, self.x_last, self.u = x, logw, x_last, u
        self.s, self.n, self.b = len(x), x[0].shape[0], x[0].shape[1]
        self.case = dict(model=model, N=self.n, B=self.b, proposal="bootstrap")
        self.has_event = x[0].dim() == 3
        self.d = x[0].shape[2] if self.has_event else 1

    def spec(self, dtype):
        """The model computing in ``dtype`` on parameters as a run in ``self.dtype`` holds them."""
        return rounded_spec(self.case, self.dtype) if dtype == torch.float64 else build_spec(self.case, dtype)

    def edited(self, logw=None, u=None):
        return History(self.model, self.dtype, self.x, self.logw if logw is None else logw, self.x_last, self.u if u is None else u)

    def soa(self, device="cuda"):
        """The library's layout: ``x_hist (S, D, B, N)``, ``logw_hist (S, B, N)``, ``x_last (D, B, N)``, ``u (S - 1, B, N)``."""
        from pyfilter_amd import ops

        x_hist = torch.stack([ops.to_soa(x.to(device), True, self.has_event) for x in self.x], 0).contiguous()
        logw = torch.stack([ops.to_cols(w.to(device)) for w in self.logw], 0).contiguous()
        x_last = ops.to_soa(self.x_last.to(device), True, self.has_event)
        u = torch.stack([ops.to_cols(v) for v in self.u.to(device).unbind(0)], 0).contiguous() if self.s > 1 else \
            torch.empty((0, self.b, self.n), dtype=self.dtype, device=device)
        return x_hist, logw, x_last, u

    def context(self):
        """(kind, packed parameter rows) of the model for ``b`` filters, through the filter's own packing."""
        from pyfilter_amd.filters.particle import SISR, proposals
        from tests.helpers import build_ssm_from_case

        filt = SISR(build_ssm_from_case(self.case, self.dtype, "cuda"), self.n, proposal=proposals.Bootstrap())
        filt.set_batch_shape(torch.Size([self.b]))
        ctx = filt._ensure_context()
        return ctx.kind, ctx.params

    def from_soa(self, out):
        """The kernel's ``(S, D, B, N)`` output as ``(S, N, B, [D])`` on the CPU."""
        from pyfilter_amd import ops

        return torch.stack([ops.from_soa(o, True, self.has_event) for o in out.unbind(0)], 0).cpu()


def _rows(x):
    return x if x.dim() == 3 else x.unsqueeze(-1)


def _make_distinct(x):
    """Particles that the rounding to the dtype made equal within a column move on by one representable value each (a pick is
    recovered from the kernel's output by exact match)."""
    r = _rows(x)
    for b in range(r.shape[1]):
        while True:
            _, inv, cnt = torch.unique(r[:, b], dim=0, return_inverse=True, return_counts=True)
            if int(cnt.max()) == 1:
                break
            order = torch.argsort(inv, stable=True)
            dup = order[1:][inv[order][1:] == inv[order][:-1]]
            r[dup, b, 0] = torch.nextafter(r[dup, b, 0], torch.full_like(r[dup, b, 0], math.inf))
    return x


def distinct(x):
    r = _rows(x)
    return all(torch.unique(r[:, b], dim=0).shape[0] == r.shape[0] for b in range(r.shape[1]))


def gather(x, idx):
    """``x (N, B, [D])`` at ``idx (M, B)``."""
    return x.gather(0, idx.unsqueeze(-1).expand(idx.shape + x.shape[2:]) if x.dim() == 3 else idx)


@functools.lru_cache(maxsize=None)
def synthetic(model, n, b, s, dtype, seed=0):
    """A history on which a backward draw is no argmax: state 0 from the model's initial law and three moves on (the Lorenz kinds: a
    tight cloud ``[1, 2, 20] + 0.05 z`` - at dt = 0.01 a particle's one-step density is otherwise so narrow that one candidate holds
    all the mass), state t + 1 = a move of state t at random ancestors, ``x_last`` likewise from the last state, log-weights
    1.5 randn.  Asserted: distinct particles per column and the input condition ``min_effective`` on the float64 oracle."""
    case = dict(model=model, N=n, B=b, proposal="bootstrap")
    spec = build_spec(case, torch.float64)
    gen = torch.Generator().manual_seed(7000 + seed)
    tail = (spec.dim,) if spec.dim > 0 else ()
    rn = lambda *sh: torch.randn(sh, generator=gen, dtype=torch.float64)  # noqa: E731
    if spec.hidden == M.HID_LORENZ63_EM:
        x = torch.tensor([1.0, 2.0, 20.0], dtype=torch.float64) + 0.05 * rn(n, b, 3)
    else:
        x = M.initial_sample(spec, rn(n, b, *tail))
        for _ in range(3):
            x = M.propagate(spec, x, rn(n, b, *tail))
    xs = [x]
    move = lambda x: M.propagate(spec, gather(x, torch.randint(n, (n, b), generator=gen)), rn(n, b, *tail))  # noqa: E731
    for _ in range(s - 1):
        xs.append(move(xs[-1]))
    x_last = move(xs[-1])
    logw = [1.5 * rn(n, b) for _ in range(s)]
    u = torch.rand((max(s - 1, 0), n, b), generator=gen, dtype=torch.float64)
    h = History(model, dtype, [_make_distinct(x.to(dtype)) for x in xs], [w.to(dtype) for w in logw], x_last.to(dtype), u.to(dtype))
    assert all(distinct(x) for x in h.x)
    if s > 1:
        eff = torch.cat([e.flatten() for e in oracle_pass(h, torch.float64)["eff"]]).median().item()
        assert eff >= min_effective(n), f"{model} {n}x{b}x{s}: a median of {eff:.1f} effective candidates per backward draw"
    return h


def edge_history(model, n, b, s, dtype, seed=1):
    """A ``synthetic`` history with the weight edges ``k_ffbs`` has code for: state 1 without mass on candidates 256..511 (a whole
    staged tile); state 0 with a NaN, a +inf and the dtype's lowest finite value on candidates 0, 1, 2 of column 0 and, in column
    1, all mass on candidate N - 1; u = 0 for trajectories 0..9 and u = 1 - eps for trajectories 10..19 at every step."""
    h = synthetic(model, n, b, s, dtype, seed)
    logw = [w.clone() for w in h.logw]
    logw[1][256:512] = -math.inf
    logw[0][:3, 0] = torch.tensor([math.nan, math.inf, torch.finfo(dtype).min], dtype=dtype)
    if b > 1:
        logw[0][: n - 1, 1] = -math.inf
    u = h.u.clone()
    u[:, :10] = 0.0
    u[:, 10:20] = 1.0 - torch.finfo(dtype).eps
    return h.edited(logw, u)


def oracle_pass(h, dtype, x_next_of=None):
    """The oracle's backward pass over ``h`` computing in ``dtype``: per step t = S - 2 .. 0 its picks ``idx (N, B)``, ``cdf_norm
    (N, B, N)`` and the effective candidate count ``1 / sum p^2`` of every draw, as lists indexed by t.  Teacher-forced from
    ``x_next_of(t + 1)`` where given (``(N, B, [D])`` in ``h.dtype``), else from its own picks."""
    spec = h.spec(dtype)
    idx, cdf, eff = [None] * (h.s - 1), [None] * (h.s - 1), [None] * (h.s - 1)
    nxt = h.x_last
    for t in range(h.s - 2, -1, -1):
        if x_next_of is not None:
            nxt = x_next_of(t + 1)
        w = cpu_ref.ffbs_sanitize_logw(h.logw[t]).to(dtype)  # (the lowest finite value of the dtype the weights are held in)
        idx[t], cdf[t] = cpu_ref.ffbs_backward_step(spec, h.x[t].to(dtype), w, nxt.to(dtype), h.u[t].to(dtype))
        p = torch.diff(cdf[t], dim=-1, prepend=torch.zeros_like(cdf[t][..., :1]))
        eff[t] = 1.0 / p.pow(2).sum(-1)
        nxt = gather(h.x[t], idx[t])
    return dict(idx=idx, cdf=cdf, eff=eff)


def recover_picks(x_t, out_t, prefer=None):
    """The candidates of ``x_t (N, B, [D])`` that the rows of ``out_t (N, B, [D])`` are bit-for-bit copies of: ``(N, B)`` int64,
    -1 where a row is no particle of the state.  Where several particles of a column hold the same value (recorded states of a
    float32 run), ``prefer (N, B)`` is named if it is one of them, else the first."""
    a, o = _rows(x_t), _rows(out_t)
    bits = {torch.float32: torch.int32, torch.float64: torch.int64}[a.dtype]
    a, o = a.contiguous().view(bits), o.contiguous().view(bits)
    pick = torch.full(o.shape[:2], -1, dtype=torch.int64)
    for b in range(a.shape[1]):
        hit = (o[:, None, b, :] == a[None, :, b, :]).all(-1)  # (N_j, N_i)
        pick[:, b] = torch.where(hit.any(-1), hit.to(torch.int64).argmax(-1), pick[:, b])
        if prefer is not None:
            pick[:, b] = torch.where(hit.gather(1, prefer[:, b : b + 1])[:, 0], prefer[:, b], pick[:, b])
    return pick


def boundary_distance(cdf_norm, u, a, b):
    """The largest ``|u - cdf_norm[k]|`` over the cdf boundaries k between picks a and b of one draw (a != b): candidate i is
    drawn for ``cdf_norm[i - 1] <= u < cdf_norm[i]``, so the boundaries between them are ``min(a, b) .. max(a, b) - 1``."""
    lo, hi = min(a, b), max(a, b)
    return float((cdf_norm[lo:hi] - float(u)).abs().max())


def compare_draws(h, picks, ref, delta, label):
    """The bars of a case: ``picks`` / ``ref["idx"]`` per step (lists of ``(N, B)``); a draw that differs from the float64 oracle
    lies within ``delta`` of every cdf boundary between the two picks, and at most ``MAX_DISAGREE`` of the case's draws differ.
    Returns ``(differing draws, draws, largest boundary distance among them)``."""
    bad, total, worst = 0, 0, 0.0
    for t in range(h.s - 1):
        assert bool((picks[t] >= 0).all()) and bool((picks[t] < h.n).all()), f"{label}: step {t} wrote a row that is no particle of state {t}"
        diff = (picks[t] != ref["idx"][t]).nonzero()
        total += picks[t].numel()
        for j, b in diff.tolist():
            dist = boundary_distance(ref["cdf"][t][j, b], h.u[t, j, b].double(), int(picks[t][j, b]), int(ref["idx"][t][j, b]))
            worst = max(worst, dist)
            bad += 1
            assert dist <= delta, (f"{label}: step {t} trajectory {j} column {b} drew candidate {int(picks[t][j, b])}, the oracle "
                                   f"{int(ref['idx'][t][j, b])}, {dist:.3e} from a cdf boundary (allowed {delta:.3e})")
    assert bad <= MAX_DISAGREE * total, f"{label}: {bad} of {total} draws differ from the float64 oracle"
    return bad, total, worst


def f32_delta(ref32, ref64, factor):
    """``factor`` x the float32 oracle's own cdf error on the case: max ``|cdf_norm(float32) - cdf_norm(float64)|``."""
    return factor * max([float((a - b).abs().max()) for a, b in zip(ref32["cdf"], ref64["cdf"])] + [0.0])


def f64_delta(n):
    """N float64 additions in another order and a rescaling of the running sum at every new maximum: N 2^-52 x 8."""
    return n * 2.0 ** -52 * 8.0
