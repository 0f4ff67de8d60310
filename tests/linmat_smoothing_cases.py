"""TEST INFRASTRUCTURE - inputs of the ``pf_smooth_ffbs_linear`` tests (``tests/test_linmat_smoothing_gpu.py``): synthetic state
histories of the ``PF_HID_LINEAR_MAT`` kind in the classes and bars of ``tests/smoothing_cases.py`` (``oracle_pass``,
``recover_picks``, ``compare_draws``, ``f32_delta``, ``f64_delta`` are used unchanged).

Parameter rows come from ``tests.linmat_cases.Case(d, 2, 4, b, y_rows=1, seed=0)``: every filter has its own row, every number is
float32-exact.  State t is a cloud ``centre_t + 0.25 min_d(s) randn(n, b, d)`` around ``centre_0 = randn(b, d)``,
``centre_{t+1} = b + A centre_t`` - not an ancestral simulation: a transition kernel of width s on a cloud of width ~1 in 8
dimensions leaves less than one effective candidate per backward draw, and a draw would only check an argmax.  ``x_last`` is a move
of the last state at random ancestors, log-weights are 1.5 randn, ``u`` is uniform; everything is generated in float64, rounded to
the dtype and made distinct per column.

Two conditions are asserted on the oracle, never on the kernel: ``min_effective(n)`` on the float64 oracle, and (float32 histories)
that the float32 oracle alone, teacher-forced with the float64 oracle's picks, differs from it in at most ``MAX_DISAGREE`` of the
case's draws."""
import functools
import math

import numpy as np
import torch

from oracle import models as M
from tests import linmat_cases as LC
from tests import linmat_oracle as LO
from tests import smoothing_cases as sc

DIMS = (1, 3, 4, 5, 8)
OBS_DIM = 2
# (N, B, S): a single particle; below one staged tile of 256 candidates; one short of / exactly / one into the second tile; a ragged
# sixth tile; S = 1 (no backward draw)
SHAPES = ((1, 2, 3), (5, 1, 2), (255, 3, 3), (256, 1, 3), (257, 2, 3), (1537, 3, 4), (300, 2, 1))
DRAW_CASES = tuple((d,) + s for d in DIMS for s in SHAPES)
EDGE_CASES = ((4, 600, 2, 3), (8, 600, 2, 3))


def spec_of_rows(rows, d, o, dtype):
    """``linmat_cases.Case.spec`` for any ``(B, NP)`` array of rows: one parameter set per filter."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
    parts = [LO.split_row(r, d, o) for r in rows]
    a, off, s, ao, bo, so = (t(np.stack([p[k] for p in parts])) for k in range(6))
    return M.ModelSpec(M.HID_LINEAR_MAT, (a, off, s), d, 1.0, None, M.OBS_LINEAR, (ao, bo, so), o)


class History(sc.History):
    """``smoothing_cases.History`` of the matrix kind: ``rows (B, NP)`` float64 numpy, float32-exact."""

    def __init__(self, rows, d, dtype, x, logw, x_last, u):
        super().__init__(f"linmat-D{d}", dtype, x, logw, x_last, u)
        self.rows, self.lin_d = rows, d
        assert self.has_event and self.d == d and rows.shape[0] == self.b

    def spec(self, dtype):
        return spec_of_rows(self.rows, self.lin_d, OBS_DIM, dtype)

    def edited(self, logw=None, u=None):
        return History(self.rows, self.lin_d, self.dtype, self.x, self.logw if logw is None else logw, self.x_last,
                       self.u if u is None else u)

    def context(self):
        """(kind, parameter rows on the GPU in the history's dtype)."""
        return LC.kernel_kind(self.lin_d, OBS_DIM), torch.from_numpy(np.ascontiguousarray(self.rows)).to(self.dtype).cuda().contiguous()


@functools.lru_cache(maxsize=None)
def synthetic(d, n, b, s, dtype, seed=0):
    case = LC.Case(d, OBS_DIM, 4, b, y_rows=1, seed=0)
    spec = case.spec(torch.float64)
    a, off, scale = spec.hidden_params
    gen = torch.Generator().manual_seed(9000 + 100 * seed + d)
    rn = lambda *sh: torch.randn(sh, generator=gen, dtype=torch.float64)  # noqa: E731
    width = 0.25 * scale.min(-1, keepdim=True)[0]  # (B, 1)
    centre = rn(b, d)
    xs = []
    for _ in range(s):
        xs.append(centre + width * rn(n, b, d))
        centre = off + (a @ centre.unsqueeze(-1)).squeeze(-1)
    x_last = M.propagate(spec, sc.gather(xs[-1], torch.randint(n, (n, b), generator=gen)), rn(n, b, d))
    logw = [1.5 * rn(n, b) for _ in range(s)]
    u = torch.rand((max(s - 1, 0), n, b), generator=gen, dtype=torch.float64)
    h = History(case.rows, d, dtype, [sc._make_distinct(x.to(dtype)) for x in xs], [w.to(dtype) for w in logw], x_last.to(dtype), u.to(dtype))
    assert torch.equal(h.spec(torch.float64).hidden_params[0], a)
    assert all(sc.distinct(x) for x in h.x)
    if s > 1:
        ref = sc.oracle_pass(h, torch.float64)
        eff = torch.cat([e.flatten() for e in ref["eff"]]).median().item()
        assert eff >= sc.min_effective(n), f"D={d} {n}x{b}x{s}: a median of {eff:.1f} effective candidates per backward draw"
        if dtype == torch.float32:
            forced = lambda t: h.x_last if t == s - 1 else sc.gather(h.x[t], ref["idx"][t])  # noqa: E731
            ref32 = sc.oracle_pass(h, torch.float32, x_next_of=forced)
            bad = sum(int((p != q).sum()) for p, q in zip(ref32["idx"], ref["idx"]))
            total = sum(p.numel() for p in ref["idx"])
            assert bad <= sc.MAX_DISAGREE * total, f"D={d} {n}x{b}x{s}: the float32 oracle differs in {bad} of {total} draws"
    return h


def edge_history(d, n, b, s, dtype, seed=1):
    """``smoothing_cases.edge_history``'s edits on a ``synthetic`` history of this kind: state 1 without mass on candidates
    256..511 (a whole staged tile); state 0 with a NaN, a +inf and the dtype's lowest finite value on candidates 0, 1, 2 of column 0
    and, in column 1, all mass on candidate N - 1; u = 0 for trajectories 0..9 and u = 1 - eps for trajectories 10..19."""
    h = synthetic(d, n, b, s, dtype, seed)
    logw = [w.clone() for w in h.logw]
    logw[1][256:512] = -math.inf
    logw[0][:3, 0] = torch.tensor([math.nan, math.inf, torch.finfo(dtype).min], dtype=dtype)
    if b > 1:
        logw[0][: n - 1, 1] = -math.inf
    u = h.u.clone()
    u[:, :10] = 0.0
    u[:, 10:20] = 1.0 - torch.finfo(dtype).eps
    return h.edited(logw, u)
