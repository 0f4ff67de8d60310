"""TEST INFRASTRUCTURE - ``tests/score_oracle.py`` for the ``PF_HID_LINEAR_MAT`` kind: a torch-CPU float64 restatement of the
transition and observation sums of the reference's ``_model_likelihood`` (``inference/batch/mcmc/proposals/gradient.py:9-32``)
for ``x' = b + A x + s e``, ``y ~ N(b_o + A_o x, diag(s_o^2))``, differentiated with torch autograd with respect to the kernels'
parameter row, and the inputs of the ``pf_path_score_linear`` tests.

    value[b]   = 1/N sum_j sum_{t=1..S-1} [ log p(x_t^j | x_{t-1}^j) + log p(y_t | x_t^j) ]
    grad[b][k] = d value[b] / d row[b][k]          row = [ A[D x D] | b[D] | s[D] | A_o[O x D] | b_o[O] | s_o[O] ]

An all-NaN observation row contributes no observation term; a partially-NaN one makes the value and the whole gradient row of its
filters NaN (``include/pf_amd.h``: pf_path_score).  ``tests/test_linmat_score_oracle_cpu.py`` holds the restatement against
``LinearModel`` and ``LinearStateSpaceModel``'s own densities.

With ``per_term`` the rows are expanded to one copy per (t, j) term before the expression is evaluated, so that autograd hands
back every term's own gradient: ``A[b][k] = 1/N sum_{t, j} |d term / d row[k]|`` - the magnitude a sum's rounding is measured
against - next to the gradient itself.  Without it the rows are one ``(B, NP)`` leaf: the expression as the reference evaluates
it, in whatever dtype."""
import torch

from tests import linmat_cases as LC
from tests.score_oracle import LOG_SQRT_2PI, MAX_CONDITION, _f32


def n_params(d: int, o: int) -> int:
    return d * d + 2 * d + o * d + 2 * o


def split(rows, d: int, o: int):
    """``rows (.., NP)`` -> ``(A (.., D, D), b (.., D), s (.., D), A_o (.., O, D), b_o (.., O), s_o (.., O))``."""
    lead = rows.shape[:-1]
    at = [0, d * d, d * d + d, d * d + 2 * d, d * d + 2 * d + o * d, d * d + 2 * d + o * d + o, n_params(d, o)]
    a, off, s, ao, bo, so = (rows[..., at[k]:at[k + 1]] for k in range(6))
    return a.reshape(lead + (d, d)), off, s, ao.reshape(lead + (o, d)), bo, so


def _terms(d, o, rows, x_prev, x_next, y):
    """``rows (.., B, NP)`` broadcastable against the terms, ``x_prev, x_next (S-1, N, B, D)``, ``y (S-1, 1, By, O)`` ->
    ``(terms (S-1, N, B), loc)``."""
    a, off, s, ao, bo, so = split(rows, d, o)
    loc = off + (a * x_prev.unsqueeze(-2)).sum(-1)
    e = (x_next - loc) / s
    trans = (-0.5 * e * e - s.log() - LOG_SQRT_2PI).sum(-1)
    missing = y.isnan().all(-1)                                              # (S-1, 1, By)
    clean = torch.where(missing.unsqueeze(-1), torch.zeros_like(y), y)
    z = (clean - (bo + (ao * x_next.unsqueeze(-2)).sum(-1))) / so
    obs = (-0.5 * z * z - so.log() - LOG_SQRT_2PI).sum(-1)
    return trans + torch.where(missing, torch.zeros_like(obs), obs), loc


def score(d: int, o: int, rows: torch.Tensor, paths: torch.Tensor, y: torch.Tensor, dtype=torch.float64, per_term: bool = True):
    """``rows (B, NP)``, ``paths (S, N, B, D)``, ``y (S-1, By, O)`` -> dict of ``value (B,)``, ``grad (B, NP)`` and, with
    ``per_term``, ``A_value (B,)``, ``A_grad (B, NP)`` - all in ``dtype`` (the dtype the expression is evaluated in)."""
    s, n, b, dd = paths.shape
    assert dd == d and rows.shape == (b, n_params(d, o)) and y.shape[0] == s - 1 and y.shape[1] in (1, b) and y.shape[2] == o
    paths, yy = paths.to(dtype), y.to(dtype).unsqueeze(1)
    leaf = rows.to(dtype)
    leaf = (leaf.expand(s - 1, n, b, leaf.shape[-1]).clone() if per_term else leaf.clone()).requires_grad_(True)
    terms, loc = _terms(d, o, leaf, paths[:-1], paths[1:], yy)
    terms.sum().backward()
    partial = (y.isnan().any(-1) & ~y.isnan().all(-1)).any(0).expand(b)      # (B,): filters with a half-observed row
    poison = torch.where(partial, torch.full((b,), float("nan"), dtype=dtype), torch.zeros(b, dtype=dtype))
    out = {"value": terms.detach().sum((0, 1)) / n + poison}
    g = leaf.grad
    out["grad"] = (g.sum((0, 1)) if per_term else g) / n + poison.unsqueeze(-1)
    if per_term:
        out["A_value"] = terms.detach().abs().sum((0, 1)) / n
        out["A_grad"] = g.abs().sum((0, 1)) / n
        x_t, loc = paths[1:], loc.detach()
        out["condition"] = float((x_t.abs() + loc.abs()).sum() / (x_t - loc).abs().sum())
        assert out["condition"] <= MAX_CONDITION, f"D{d}-O{o}: inputs conditioned {out['condition']:.3g} > {MAX_CONDITION:g}"
    return out


class Inputs:
    """One ``pf_path_score_linear`` call: ``rows (B, NP)`` as ``linmat_cases.Case`` draws them (float32-exact, one row per filter),
    ``paths (S, N, B, D)`` simulated from the model itself from a level-1 start, ``y (S-1, By, O)`` simulated from path 0 of filter
    0 (or of every filter) - values that are exact in float32."""

    def __init__(self, d: int, o: int, s: int, n: int, b: int, by: int = 1, seed: int = 0):
        assert by in (1, b)
        self.d, self.o, self.s, self.n, self.b, self.by = d, o, s, n, b, by
        self.rows = rows = torch.from_numpy(LC.Case(d, o, 4, b, y_rows=by, seed=seed).rows.copy())
        gen = torch.Generator().manual_seed(7100 + seed)
        a, off, sc, ao, bo, so = split(rows, d, o)
        x = 1.0 + 0.1 * torch.randn((n, b, d), generator=gen, dtype=torch.float64)
        xs = [x]
        for _ in range(s - 1):
            x = off + (a * x.unsqueeze(-2)).sum(-1) + sc * torch.randn((n, b, d), generator=gen, dtype=torch.float64)
            xs.append(x)
        self.paths = _f32(torch.stack(xs, 0))
        xo = self.paths[1:, 0, :by]                                            # (S-1, By, D)
        noise = torch.randn((s - 1, by, o), generator=gen, dtype=torch.float64)
        self.y = _f32(bo[:by] + (ao[:by] * xo.unsqueeze(-2)).sum(-1) + so[:by] * noise)

    def soa(self, dtype, device):
        """The kernel's layouts: ``(rows (B, NP), paths (S, D, B, N), y (S-1, By, O))``."""
        to = lambda t: t.to(device=device, dtype=dtype).contiguous()  # noqa: E731
        return to(self.rows), to(self.paths.permute(0, 3, 2, 1)), to(self.y)
