"""TEST INFRASTRUCTURE - a torch-CPU restatement of the transition and observation sums of the reference's ``_model_likelihood``
(``inference/batch/mcmc/proposals/gradient.py:9-32``) for the built-in model kinds, differentiated with torch autograd with
respect to the kernels' parameter rows, and the inputs of the path-score tests.

    value[b]   = 1/N sum_j sum_{t=1..S-1} [ log p(x_t^j | x_{t-1}^j) + log p(y_t | x_t^j) ]
    grad[b][k] = d value[b] / d row[b][k]          row = [ hp0[D] hp1[D] hp2[D] hp3[D] | A[O x D] | b[O] | s[O] ]

``(loc, scale)`` come from the package's own torch ``mean_scale`` callables (``pyfilter_amd.timeseries.models``), applied per
component; the transition density is ``N(loc, |scale| inc)`` and the observation ``N(b + A x, s)`` or ``N(mu, x)`` (PF_OBS_SV),
as ``LinearStateSpaceModel`` / ``StochasticVolatilityModel`` define them (``tests/test_score_oracle_cpu.py`` holds the
restatement against those classes).  An all-NaN observation row contributes no observation term; a partially-NaN one makes the
value and the whole gradient row of its filters NaN (``include/pf_amd.h``: pf_path_score).

With ``per_term`` the rows are expanded to one copy per (t, j) term before the expression is evaluated, so that autograd hands
back every term's own gradient: ``A[b][k] = 1/N sum_{t, j} |d term / d row[k]|`` - the magnitude a sum's rounding is measured
against - next to the gradient itself (their signed sum).  Without it the rows are one ``(B, NP)`` leaf: the expression as the
reference evaluates it, in whatever dtype."""
import math

import torch

from pyfilter_amd import _lib as L
from pyfilter_amd.timeseries import TimeseriesState, models

LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
HIDDEN = {"linear": L.HID_LINEAR, "sine": L.HID_SINE_EM, "verhulst": L.HID_VERHULST_EM, "lorenz": L.HID_LORENZ63_EM, "ou": L.HID_OU}
DT = {"linear": 1.0, "sine": 0.1, "verhulst": 0.1, "lorenz": 0.01, "ou": 1.0}
MAX_CONDITION = 1e3  # sum (|x_t| + |loc|) / sum |x_t - loc|: the cancellation the float64 tolerance allows for


class Kind:
    """What ``pf_model`` says about a model (the attributes of ``timeseries.KernelKind``)."""

    def __init__(self, name: str, dim: int, obs_dim: int, sv: bool = False):
        self.name, self.hid_kind, self.dim, self.obs_dim = name, HIDDEN[name], dim, obs_dim
        self.obs_kind = L.OBS_SV if sv else L.OBS_LINEAR
        self.dt = DT[name]
        self.inc_scale = 1.0 if name in ("linear", "ou") else math.sqrt(self.dt)
        self.is_user = False

    @classmethod
    def of(cls, kernel_kind) -> "Kind":
        """The same description read off a model's ``kernel_kind`` (its own ``dt`` and increment scale)."""
        name = next(k for k, v in HIDDEN.items() if v == kernel_kind.hid_kind)
        kind = cls(name, kernel_kind.dim, kernel_kind.obs_dim, kernel_kind.obs_kind == L.OBS_SV)
        kind.dt, kind.inc_scale = float(kernel_kind.dt), float(kernel_kind.inc_scale)
        return kind

    @property
    def n_params(self) -> int:
        return 4 * self.dim + self.obs_dim * self.dim + 2 * self.obs_dim

    def __repr__(self):
        return f"{self.name}-D{self.dim}-O{self.obs_dim}-{'sv' if self.obs_kind == L.OBS_SV else 'lin'}"


def _package_mean_scale(kind):
    """The package's torch ``mean_scale`` of the kind, as ``f(x (.., D), hp (4, .., D)) -> (loc, scale)`` applied per component."""
    dt = kind.dt
    hid = kind.hid_kind
    if hid == L.HID_LINEAR:
        proc, n = models.AR(0.0, 0.0, 1.0), 3
    elif hid == L.HID_SINE_EM:
        proc, n = models.SineDiffusion(0.0, 1.0, dt=dt), 2
    elif hid == L.HID_VERHULST_EM:
        proc, n = models.Verhulst(1.0, 1.0, 1.0, dt=dt), 3
    elif hid == L.HID_OU:
        proc, n = models.OrnsteinUhlenbeck(1.0, 1.0, 1.0, dt=dt), 3
    elif hid == L.HID_LORENZ63_EM:
        proc = models.Lorenz63(1.0, 1.0, 1.0, dt=dt)

        def lorenz(x, hp):  # (s, r, b live in component 0 of hp0 .. hp2, sigma_d in hp3)
            return proc._mean_scale(TimeseriesState(0, x, torch.Size([3])), hp[0][..., 0], hp[1][..., 0], hp[2][..., 0], hp[3])

        return lorenz
    else:
        raise ValueError(hid)

    def elementwise(x, hp):
        return proc._mean_scale(TimeseriesState(0, x, torch.Size([])), *hp[:n])

    return elementwise


def _terms(kind, rows, x_prev, x_next, y):
    """``rows (.., B, NP)`` broadcastable against the terms, ``x_prev, x_next (S-1, N, B, D)``, ``y (S-1, 1, By, O)`` ->
    ``(terms (S-1, N, B), loc)``."""
    d, o = kind.dim, kind.obs_dim
    hp = [rows[..., k * d:(k + 1) * d] for k in range(4)]
    a = rows[..., 4 * d:4 * d + o * d].reshape(rows.shape[:-1] + (o, d))
    ob, os_ = rows[..., 4 * d + o * d:4 * d + o * d + o], rows[..., 4 * d + o * d + o:4 * d + o * d + 2 * o]
    loc, scale = _package_mean_scale(kind)(x_prev, hp)
    loc, scale = torch.broadcast_tensors(loc, scale)
    e = (x_next - loc) / (scale * kind.inc_scale)
    trans = (-0.5 * e * e - math.log(kind.inc_scale) - LOG_SQRT_2PI - scale.abs().log()).sum(-1)
    missing = y.isnan().all(-1)                                              # (S-1, 1, By)
    clean = torch.where(missing.unsqueeze(-1), torch.zeros_like(y), y)
    if kind.obs_kind == L.OBS_SV:
        m, s = ob, x_next[..., :1]
    else:
        m, s = ob + (a * x_next.unsqueeze(-2)).sum(-1), os_
    m, s = torch.broadcast_tensors(m, s)
    z = (clean - m) / s
    obs = (-0.5 * z * z - s.log() - LOG_SQRT_2PI).sum(-1)
    return trans + torch.where(missing, torch.zeros_like(obs), obs), loc


def score(kind, rows: torch.Tensor, paths: torch.Tensor, y: torch.Tensor, dtype=torch.float64, per_term: bool = True):
    """``rows (B, NP)``, ``paths (S, N, B, D)``, ``y (S-1, By, O)`` -> dict of ``value (B,)``, ``grad (B, NP)`` and, with
    ``per_term``, ``A_value (B,)``, ``A_grad (B, NP)`` - all in ``dtype`` (the dtype the expression is evaluated in)."""
    s, n, b, d = paths.shape
    assert d == kind.dim and rows.shape == (b, kind.n_params) and y.shape[0] == s - 1 and y.shape[1] in (1, b) and y.shape[2] == kind.obs_dim
    paths, yy = paths.to(dtype), y.to(dtype).unsqueeze(1)
    leaf = rows.to(dtype)
    leaf = (leaf.expand(s - 1, n, b, leaf.shape[-1]).clone() if per_term else leaf.clone()).requires_grad_(True)
    terms, loc = _terms(kind, leaf, paths[:-1], paths[1:], yy)
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
        assert out["condition"] <= MAX_CONDITION, f"{kind}: inputs conditioned {out['condition']:.3g} > {MAX_CONDITION:g}"
    return out


# ----------------------------------------------------------------------------------------------------------------
# inputs: trajectories simulated from the model itself (realistic residuals), float64 values that are exact in float32
# ----------------------------------------------------------------------------------------------------------------
def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.float().double()


def base_rows(kind, b: int, gen: torch.Generator) -> torch.Tensor:
    """``(B, NP)`` parameter rows: the kind's values with a few per cent of per-filter spread; the slots a kind never reads hold
    7.0 (their gradient must come out as exactly 0).  Transition scales are at least 0.05."""
    d, o = kind.dim, kind.obs_dim
    sv = kind.obs_kind == L.OBS_SV
    hp = torch.full((4, d), 7.0, dtype=torch.float64)
    comp = 1.0 + 0.1 * torch.arange(d, dtype=torch.float64)  # (components differ)
    if kind.name == "linear":
        hp[0], hp[1], hp[2] = 0.1 * comp, 0.9, (0.075 if sv else 0.3) * comp
    elif kind.name == "sine":
        hp[0], hp[1] = 0.5 * comp, (0.2 if sv else 0.4) * comp
    elif kind.name == "verhulst":
        hp[0], hp[1], hp[2] = 1.0 * comp, 1.0, 0.3 * comp
    elif kind.name == "ou":
        hp[0], hp[1], hp[2] = 0.5 * comp, 1.0, (0.1 if sv else 0.4) * comp
    else:  # lorenz
        hp[0, 0], hp[1, 0], hp[2, 0], hp[3] = 10.0, 28.0, 8.0 / 3.0, torch.tensor([1.0, 1.2, 0.8], dtype=torch.float64)
    a = 0.6 + 0.4 * torch.randn((o, d), generator=gen, dtype=torch.float64)
    if sv:
        a = torch.full((o, d), 0.0, dtype=torch.float64)  # (pack_params' row for the SV observation: A = 0, b = mu, s = 1)
    ob = torch.full((o,), 0.05 if sv else 0.1, dtype=torch.float64)
    os_ = torch.full((o,), 1.0 if sv else 0.5, dtype=torch.float64) * (1.0 if sv else 1.0 + 0.2 * torch.arange(o, dtype=torch.float64))
    row = torch.cat([hp.reshape(-1), a.reshape(-1), ob, os_])
    spread = 1.0 + 0.05 * (2.0 * torch.rand((b, row.numel()), generator=gen, dtype=torch.float64) - 1.0)
    rows = row * spread
    if sv:  # (the slots of the SV row that are constants stay constants)
        rows[:, 4 * d:4 * d + o * d] = 0.0
        rows[:, 4 * d + o * d + o:] = 1.0
    return _f32(rows)


def start_level(kind, b: int) -> torch.Tensor:
    """Where the kind's trajectories live, ``(D,)``: levels of order 1, Lorenz-63 on its attractor (order 20)."""
    if kind.name == "lorenz":
        return torch.tensor([-5.91652, -5.52332, 24.5723], dtype=torch.float64)
    if kind.name == "sine":
        return 0.5 * (1.0 + 0.1 * torch.arange(kind.dim, dtype=torch.float64)) + math.pi  # (the attracting zero of sin(x - gamma))
    return torch.ones(kind.dim, dtype=torch.float64)


class Inputs:
    """One ``pf_path_score`` call: ``rows (B, NP)``, ``paths (S, N, B, D)``, ``y (S-1, By, O)`` from a CPU generator."""

    def __init__(self, kind, s: int, n: int, b: int, by: int = 1, seed: int = 0):
        assert by in (1, b)
        self.kind, self.s, self.n, self.b, self.by = kind, s, n, b, by
        gen = torch.Generator().manual_seed(7000 + seed)
        d, o = kind.dim, kind.obs_dim
        self.rows = rows = base_rows(kind, b, gen)
        hp = [rows[:, k * d:(k + 1) * d] for k in range(4)]
        ms = _package_mean_scale(kind)
        x = start_level(kind, b) + (0.5 if kind.name == "lorenz" else 0.1) * torch.randn((n, b, d), generator=gen, dtype=torch.float64)
        xs = [x]
        for _ in range(s - 1):
            loc, scale = ms(x, hp)
            x = loc + scale * kind.inc_scale * torch.randn((n, b, d), generator=gen, dtype=torch.float64)
            xs.append(x)
        self.paths = _f32(torch.stack(xs, 0))
        if kind.name == "verhulst" or kind.obs_kind == L.OBS_SV:
            assert bool((self.paths > 0).all()), f"{kind}: a trajectory left the positive half-line"
        # the observations of one trajectory per series (particle 0 of filter 0, or of every filter)
        xo = self.paths[1:, 0, :by]                                            # (S-1, By, D)
        a = rows[:by, 4 * d:4 * d + o * d].reshape(by, o, d)
        ob, os_ = rows[:by, 4 * d + o * d:4 * d + o * d + o], rows[:by, 4 * d + o * d + o:]
        noise = torch.randn((s - 1, by, o), generator=gen, dtype=torch.float64)
        if kind.obs_kind == L.OBS_SV:
            self.y = _f32(ob + xo[..., :1] * noise)
        else:
            self.y = _f32(ob + (a * xo.unsqueeze(-2)).sum(-1) + os_ * noise)

    def soa(self, dtype, device):
        """The kernel's layouts: ``(rows (B, NP), paths (S, D, B, N), y (S-1, By, O))``."""
        to = lambda t: t.to(device=device, dtype=dtype).contiguous()  # noqa: E731
        return to(self.rows), to(self.paths.permute(0, 3, 2, 1)), to(self.y)
