"""TEST INFRASTRUCTURE - the inputs, the covariance oracle and the error measures of the ``pf_forecast_linear`` tests
(``tests/test_forecast_linear_cpu.py``, ``tests/test_forecast_linear_gpu.py``).

Inputs: the parameter rows and the cloud of ``tests/linmat_cases.Case(d, o, n, b, y_rows=b, level=...)`` (every filter its own row);
tapes ``z (H, N, B, D)``, ``e (H, N, B, O)`` and the weights from a seeded generator, every number float32-exact, the three kinds of
weights of ``tests/forecast_oracle.Inputs``.  Moments and paths: ``tests.forecast_oracle.forecast`` as it stands.  Covariances:
``covariances`` below, with the same conventions - model arithmetic in the inputs' dtype, sums in float64, centred, weights as given:

    x_cov = sum W (x - x_mean)(x - x_mean)^T          y_cov = sum W (m - y_mean)(m - y_mean)^T + diag(sum W s^2)

Error measures, per array group (``group_errors``): means and paths ``max |d| / (1 + |ref|)``; variances and covariances
``max |d_ij| / sqrt(ref_ii ref_jj)`` (a variance: relative to itself; where that scale is 0 the entry must be met exactly).
Float32 bar (``f32_bars``): four times what ``oracle/models.py`` evaluated in float32 differs from its float64 self on exactly
those inputs - the margin of the nested and forecast bars - plus a floor of ``64 eps32`` (``linmat_cases.bounds``'s); computed
from the oracle alone, never from the kernel."""
import ctypes as C
import functools

import numpy as np
import torch

from oracle import models as M
from tests import forecast_oracle as FO
from tests import linmat_cases as LC

EPS32 = LC.EPS32
WEIGHTS = FO.WEIGHTS
KEYS = FO.KEYS + ("x_cov", "y_cov")
GROUPS = ("means", "seconds", "paths")
EDGE_SHAPES = LC.EDGE_SHAPES
EDGE_B = (1, 3)
EDGE_H = (1, 7)
F64_BAR = 1e-9
F32_FLOOR = 64.0 * EPS32
F32_MARGIN = 4.0


def covariances(spec, x, w, z):
    """``x (N, B, [D])``, ``w (N, B)`` or None (1 / N), ``z (H, N, B, [D])`` -> ``(x_cov (H, B, D, D), y_cov (H, B, O, O))`` in the
    inputs' dtype (a scalar state or observation: ``(H, B, 1, 1)``)."""
    dtype = x.dtype
    ww = (torch.full(x.shape[:2], 1.0 / x.shape[0], dtype=torch.float64) if w is None else w.double()).unsqueeze(-1)
    xc, yc = [], []
    for h in range(z.shape[0]):
        x = M.propagate(spec, x, z[h])
        m, s = M.obs_loc_scale(spec, x)
        s = M._t(s, m).expand(m.shape)
        if spec.obs_dim == 0:
            m, s = m.unsqueeze(-1), s.unsqueeze(-1)
        out = []
        for first in (x if spec.dim > 0 else x.unsqueeze(-1), m):
            f = first.double()
            c = f - (ww * f).sum(0)
            out.append((ww.unsqueeze(-1) * (c.unsqueeze(-1) * c.unsqueeze(-2))).sum(0))  # (c_i c_j first: the same bits both ways)
        xc.append(out[0].to(dtype))
        yc.append((out[1] + torch.diag_embed((ww * (s * s).double()).sum(0))).to(dtype))
    return torch.stack(xc, 0), torch.stack(yc, 0)


def full_oracle(spec, x, w, z, e):
    res = FO.forecast(spec, x, w, z, e)
    res["x_cov"], res["y_cov"] = covariances(spec, x, w, z)
    return res


class Inputs:
    """One forecast call on a ``linmat_cases`` case: float64 tensors whose values are exact in float32."""

    def __init__(self, d, o, n, b, h, weights="random", level=0.0, seed=0):
        self.d, self.o, self.n, self.b, self.h, self.weights, self.level = d, o, n, b, h, weights, level
        self.case = LC.case(d, o, n, b, b, level=level)
        gen = torch.Generator().manual_seed(7000 + 97 * seed + 13 * d + o)
        rn = lambda *s: torch.randn(s, generator=gen, dtype=torch.float32).double()  # noqa: E731
        self.x = torch.from_numpy(np.ascontiguousarray(self.case.x))
        self.z, self.e = rn(h, n, b, d), rn(h, n, b, o)
        if weights == "none":
            self.w = None
        else:
            w = torch.softmax(rn(n, b), dim=0)
            if weights == "half_zero":  # filter 0: every second weight exactly 0 (the first particle keeps its: N = 1)
                w[1::2, 0] = 0.0
                w[:, 0] = w[:, 0] / w[:, 0].sum()
            self.w = w.float().double()
        self._ref = {}

    def __repr__(self):
        return f"D{self.d}-O{self.o} {self.n}x{self.b} H={self.h} W={self.weights}" + (f" level={self.level:g}" if self.level else "")

    def reference(self):
        """The float64 oracle (the parameter rows are float32-exact: a run in either dtype holds the same parameters)."""
        if "f64" not in self._ref:
            self._ref["f64"] = full_oracle(self.case.spec(torch.float64), self.x, self.w, self.z, self.e)
        return self._ref["f64"]

    def oracle_f32(self):
        """``oracle/models.py`` evaluated in float32 on these inputs (sums in float64, results returned in float32)."""
        if "f32" not in self._ref:
            f = lambda t: None if t is None else t.float()  # noqa: E731
            self._ref["f32"] = full_oracle(self.case.spec(torch.float32), f(self.x), f(self.w), f(self.z), f(self.e))
        return self._ref["f32"]

    def f32_bars(self):
        return {g: F32_MARGIN * v + F32_FLOOR for g, v in group_errors(self.oracle_f32(), self.reference()).items()}


@functools.lru_cache(maxsize=None)
def inputs(*args, **kwargs):
    return Inputs(*args, **kwargs)


# ---- error measures ----------------------------------------------------------------------------------------------------------------
def _second_error(got, ref, scale):
    err = (got.double().cpu() - ref.double()).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    zero = scale == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    return float((err[~zero] / scale[~zero]).max()) if bool((~zero).any()) else 0.0


def group_errors(got, ref):
    """``{"means", "seconds", "paths"}``: the worst scaled error of each array group (module docstring); ``got`` may lack paths or
    covariances (None): those are skipped."""
    out = {"means": max(FO.scaled_error(got[k], ref[k]) for k in ("x_mean", "y_mean"))}
    worst = 0.0
    for var, cov in (("x_var", "x_cov"), ("y_var", "y_cov")):
        v = ref[var].double()
        worst = max(worst, _second_error(got[var], ref[var], v))
        if got.get(cov) is not None:
            worst = max(worst, _second_error(got[cov], ref[cov], (v.unsqueeze(-1) * v.unsqueeze(-2)).sqrt()))
    out["seconds"] = worst
    out["paths"] = max([FO.scaled_error(got[k], ref[k]) for k in ("x_path", "y_path") if got.get(k) is not None] or [0.0])
    return out


# ---- the case lists ------------------------------------------------------------------------------------------------------------------
def tile(d, covariance=False):
    """Particles per workgroup of the part kernel for state dimension ``d``, derived from ``pf_forecast_linear_workspace_bytes``:
    the largest ``N`` that still takes one tile's worth of workspace."""
    from pyfilter_amd import _lib as L

    def nbytes(n):
        out = C.c_size_t(0)
        L.check(L.load().pf_forecast_linear_workspace_bytes(n, 1, 1, d, 1, int(covariance), C.byref(out)), "pf_forecast_linear_workspace_bytes")
        return out.value

    one = nbytes(1)
    lo, hi = 1, 1 << 20  # nbytes(lo) == one < nbytes(hi)
    assert nbytes(hi) > one
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if nbytes(mid) == one else (lo, mid)
    return lo


def edge_n(t, items):
    """1, one below / at / one above the tile, three tiles plus a ragged tail with ``N % items != 0``"""
    tail = 3 * t + 2 * items + 1
    assert tail % items != 0 or items == 1
    return (1, t - 1, t, t + 1, tail)


def edge_inputs(d, o, tile_d, items):
    """The edge calls of one shape: every N edge x B x H x kind of weights"""
    return [inputs(d, o, n, b, h, weights, seed=k) for n in edge_n(tile_d, items) for b in EDGE_B for h in EDGE_H
            for k, weights in enumerate(WEIGHTS)]


# The tile sizes the edge lists are built with where no GPU library can be asked (the CPU checks of the float32 cases): the GPU test
# asserts that they are what ``tile`` derives from the library, so the CPU conditions cover exactly the GPU cases.
ASSUMED_TILE = {d: 256 * (4 if d <= 4 else 2) for d in range(1, 9)}
ASSUMED_ITEMS = {d: ASSUMED_TILE[d] // 256 for d in range(1, 9)}


def level_inputs():
    return [inputs(d, o, 65, 3, h, WEIGHTS[k % 3], level=lv, seed=k % 3) for d, o in LC.LEVEL_SHAPES for lv in LC.LEVELS
            for k, h in enumerate(EDGE_H)]


# float32 cases that left the list because the oracle's own float32 run does not meet the conditions the bar rests on
# (tests/test_forecast_linear_cpu.py::test_float32_cases_meet_the_conditions_of_their_bar): none.
F32_EXCLUDED = ()


def float32_inputs():
    cases = [i for d, o in EDGE_SHAPES for i in edge_inputs(d, o, ASSUMED_TILE[d], ASSUMED_ITEMS[d])] + level_inputs()
    return [i for i in cases if repr(i) not in F32_EXCLUDED]


# ---- the package's models on these inputs ---------------------------------------------------------------------------------------------
def linear_ssm(inp, dtype, device):
    """The case's model as a ``LinearModel`` under a ``LinearStateSpaceModel``, every filter its own parameters"""
    from torch.distributions import Independent, Normal

    from pyfilter_amd import timeseries as ts

    spec = inp.case.spec(dtype)
    to = lambda t: t.to(device)  # noqa: E731
    a, off, s = (to(p) for p in spec.hidden_params)
    ao, bo, so = (to(p) for p in spec.obs_params)
    d, o = inp.d, inp.o
    zero, one = torch.zeros(d, dtype=dtype, device=device), torch.ones(d, dtype=dtype, device=device)
    inc = Independent(Normal(zero[0], one[0]).expand(torch.Size([d])), 1)
    hidden = ts.LinearModel((a, off, s), inc, lambda *_: Independent(Normal(zero, one), 1))
    return ts.LinearStateSpaceModel(hidden, (ao, bo, so), torch.Size([o]))


def filter_state(inp, ssm, dtype, device):
    """A ``ParticleFilterCorrection`` holding the inputs' cloud and the logarithms of its weights (``none``: equal weights)"""
    from pyfilter_amd.filters.particle.state import ParticleFilterCorrection
    from pyfilter_amd.timeseries import TimeseriesState

    x = inp.x.to(device=device, dtype=dtype)
    log_w = (torch.zeros(inp.n, inp.b, dtype=torch.float64) if inp.w is None else inp.w.log()).to(device=device, dtype=dtype)
    return ParticleFilterCorrection(TimeseriesState(0, x, ssm.hidden.event_shape), log_w, torch.zeros(inp.b, dtype=dtype, device=device),
                                    torch.arange(inp.n, device=device).unsqueeze(-1).expand(inp.n, inp.b))


TRACKER_F = [[1.0, 0, 1, 0], [0, 1, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1]]  # (x, y, vx, vy): README's constant-velocity tracker
TRACKER_H = [[1.0, 0, 0, 0], [0, 1, 0, 0]]
TRACKER_G = [0.5, 0.5, 1.0, 1.0]


def tracker_builder(dtype, device):
    """``build(theta)`` of README's tracker: ``theta["q"]``, ``theta["r"]`` of shape ``(B,)``"""
    from torch.distributions import Independent, Normal

    from pyfilter_amd import timeseries as ts

    kw = dict(dtype=dtype, device=device)
    f, hm, g = torch.tensor(TRACKER_F, **kw), torch.tensor(TRACKER_H, **kw), torch.tensor(TRACKER_G, **kw)
    inc = Independent(Normal(torch.tensor(0.0, **kw), torch.tensor(1.0, **kw)).expand(torch.Size([4])), 1)
    x0 = lambda *_: Independent(Normal(torch.zeros(4, **kw), torch.ones(4, **kw)), 1)  # noqa: E731

    def build(theta):
        s = theta["q"].reshape(-1, 1) * g
        hidden = ts.LinearModel((f, torch.zeros_like(s), s), inc, x0)
        return ts.LinearStateSpaceModel(hidden, (hm, torch.zeros(2, **kw), theta["r"].reshape(-1, 1) * torch.ones(2, **kw)), torch.Size([2]))

    return build


def forecast_dict(fc):
    out = FO.as_dict(fc)
    out["x_cov"], out["y_cov"] = fc.x_covariance, fc.y_covariance
    return out


# ---- running the kernel ---------------------------------------------------------------------------------------------------------------
def run_kernel(inp, dtype=torch.float64, paths=True, covariance=True, tapes=True, seed=11):
    """``pf_forecast_linear`` on the inputs - ``tapes = False``: on its own Philox draws - as a dict like the oracle's (reference
    layouts), on the device."""
    from pyfilter_amd import ops

    to = lambda t: None if t is None else t.to(device="cuda", dtype=dtype)  # noqa: E731
    rows = to(torch.from_numpy(np.ascontiguousarray(inp.case.rows))).contiguous()
    soa = ops.to_soa(to(inp.x), True, True)
    tape = lambda t: to(t).permute(0, 3, 2, 1).contiguous() if tapes else None  # noqa: E731
    xm, xv, ym, yv, xc, yc, xp, yp = ops.forecast_linear_soa(LC.kernel_kind(inp.d, inp.o), rows, inp.h, soa,
                                                             None if inp.w is None else ops.to_cols(to(inp.w)), tape(inp.z), tape(inp.e),
                                                             seed, paths, covariance)
    torch.cuda.synchronize()
    view = lambda p: None if p is None else p.permute(0, 3, 2, 1)  # noqa: E731
    return dict(zip(KEYS, (xm, xv, ym, yv, view(xp), view(yp), xc, yc)))
