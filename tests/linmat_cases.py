"""The case list of the ``PF_HID_LINEAR_MAT`` parity tests (``tests/test_linmat_oracle_cpu.py``, ``tests/test_linmat_parity_gpu.py``,
``tools/linmat_parity.py``): inputs from a seeded numpy generator, every number float32-exact so that both dtypes see the same inputs.

Per filter: ``A = 0.9 I + 0.1 R / sqrt(D)`` (R standard normal), ``b`` and ``b_o`` 0.1 x standard normal, ``s`` uniform in [0.3, 0.6],
``A_o`` standard normal, ``s_o = ratio x`` (uniform in [0.3, 0.6]).  A true state at ``level`` (+ standard normal) makes one
transition and is observed: ``y`` is simulated from the model, and the particles are the true state + 0.3 x standard normal, so every
residual is O(1) standard deviations of its law.  Every filter has its own parameter row - and, with ``y_rows = B``, its own true
state and observation - so a kernel that read filter 0's row for everybody is off by O(1)."""
import functools

import numpy as np
import torch

from oracle import cpu_ref
from oracle import models as M
from tests import linmat_oracle as LO

EPS32 = float(np.finfo(np.float32).eps)
ENTRY_POINTS = ("lgo", "bootstrap", "pre_lgo", "pre_bootstrap", "propagate")
COND_CAP = 1e8  # beyond it the float64 bound is no test of the kernel: its loss is cond(P) eps by construction


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


class Case:
    def __init__(self, d, o, n, b, y_rows=1, ratio=2.0, level=0.0, seed=0):
        assert y_rows in (1, b)
        self.d, self.o, self.n, self.b, self.y_rows, self.ratio, self.level, self.seed = d, o, n, b, y_rows, ratio, level, seed
        g = np.random.default_rng([d, o, n, b, y_rows, int(round(1e6 * ratio)), int(level), seed])
        rows, truth, ys = [], [], []
        for _ in range(b):
            a = f32(0.9 * np.eye(d) + 0.1 * g.standard_normal((d, d)) / np.sqrt(d))
            off, s = f32(0.1 * g.standard_normal(d)), f32(g.uniform(0.3, 0.6, d))
            ao, bo, so = f32(g.standard_normal((o, d))), f32(0.1 * g.standard_normal(o)), f32(ratio * g.uniform(0.3, 0.6, o))
            x_true = level + g.standard_normal(d)
            x_next = off + a @ x_true + s * g.standard_normal(d)
            rows.append(LO.pack_row(a, off, s, ao, bo, so))
            truth.append(x_true)
            ys.append(bo + ao @ x_next + so * g.standard_normal(o))
        self.rows = np.stack(rows)                                   # (B, NP)
        centre = np.stack(truth if y_rows == b else [truth[0]] * b)  # (a shared observation: one true state for every filter)
        self.y = f32(np.stack(ys)[:y_rows])                          # (y_rows, O)
        self.x = f32(centre[None] + 0.3 * g.standard_normal((n, b, d)))  # (N, B, D)
        self.z = f32(g.standard_normal((n, b, d)))

    def __repr__(self):
        return f"D{self.d}-O{self.o}-N{self.n}-B{self.b}-y{self.y_rows}-r{self.ratio:g}-x{self.level:g}"

    # ---- the exact oracle ----
    @functools.lru_cache(maxsize=None)
    def oracle(self, entry):
        if entry in ("lgo", "bootstrap"):
            return LO.sample_and_weight(self.rows, self.y, self.x, self.z, self.d, self.o, entry)
        if entry == "propagate":
            return LO.sample_and_weight(self.rows, None, self.x, self.z, self.d, self.o, "bootstrap", weigh=False)
        return LO.pre_weight(self.rows, self.y, self.x, self.d, self.o, entry[4:])

    def cond_P(self):
        return max(LO.constants(r, self.d, self.o)["cond_P"] for r in self.rows)

    # ---- the reference's own arithmetic (oracle/cpu_ref.py) in torch, float64 or float32, on the CPU ----
    def spec(self, dtype):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
        parts = [LO.split_row(r, self.d, self.o) for r in self.rows]
        a, off, s, ao, bo, so = (t(np.stack([p[k] for p in parts])) for k in range(6))
        return M.ModelSpec(M.HID_LINEAR_MAT, (a, off, s), self.d, 1.0, None, M.OBS_LINEAR, (ao, bo, so), self.o)

    @functools.lru_cache(maxsize=None)
    def reference(self, entry, dtype):
        """``(x (N, B, D) | None, w (N, B) | None)`` as float64 numpy arrays."""
        spec = self.spec(dtype)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
        x, z = t(self.x), t(self.z)
        y = t(self.y[0] if self.y_rows == 1 else self.y)
        if entry == "lgo":
            xn, w = cpu_ref.lgo_sample_and_weight(spec, y, x, z)
        elif entry == "bootstrap":
            xn, w = cpu_ref.bootstrap_sample_and_weight(spec, y, x, z)
        elif entry == "propagate":
            xn, w = M.propagate(spec, x, z), None
        elif entry == "pre_lgo":
            xn, w = None, cpu_ref.lgo_pre_weight(spec, y, x)
        else:
            xn, w = None, cpu_ref.default_pre_weight(spec, y, x)
        return tuple(None if v is None else v.double().numpy() for v in (xn, w))

    def reference_completes_in_float32(self):
        """The reference's float32 run factorises a positive-definite covariance (both of them) and returns finite numbers."""
        spec = self.spec(torch.float32)
        a, _, s = spec.obs_params
        hs = spec.hidden_params[2]
        cov = (torch.diag_embed(hs.pow(-2.0)) + a.transpose(-2, -1) @ torch.diag_embed(s.pow(-2.0)) @ a).inverse()
        inn = torch.diag_embed(s.pow(2.0)) + a @ torch.diag_embed(hs.pow(2.0)) @ a.transpose(-2, -1)
        ok = all(bool((torch.linalg.cholesky_ex(m).info == 0).all()) for m in (cov, inn))
        return ok and all(np.isfinite(v).all() for e in ENTRY_POINTS for v in self.reference(e, torch.float32) if v is not None)

    # ---- the bounds ----
    def bounds(self, entry, dtype):
        """``(tol_x | None, tol_w | None)``.  float64: ``linmat_oracle.bounds_f64``.  float32: four times the error of the reference's
        own float32 arithmetic against the exact oracle - the maximum over the particles of the case, per state component - plus a
        floor of ``64 eps32`` x the oracle's magnitudes; computed from the reference, never from the kernel."""
        res = self.oracle(entry)
        if dtype == torch.float64:
            return LO.bounds_f64(res, self.d)
        rx, rw = self.reference(entry, torch.float32)
        tol_x = tol_w = None
        if rx is not None:
            tol_x = 4.0 * np.abs(rx - res["x"]).max(axis=(0, 1), keepdims=True) + 64.0 * EPS32 * res["mag_x"]
        if rw is not None:
            tol_w = 4.0 * np.abs(rw - res["w"]).max() + 64.0 * EPS32 * res["A_w"]
        return tol_x, tol_w


@functools.lru_cache(maxsize=None)
def case(*args, **kwargs):
    return Case(*args, **kwargs)


ALL_SHAPES = [(d, o) for d in range(1, 9) for o in range(1, 9)]
EDGE_SHAPES = [(4, 2), (8, 8), (7, 1), (3, 5)]
EDGE_N = (1, 63, 64, 65, 255, 256, 257, 1025)
EDGE_B_ROWS = ((1, 1), (3, 1), (3, 3))  # (B, y_rows)
SECOND_TRIP_N = 2048 * 256 + 77  # the element-wise grid is capped at 2048 workgroups of 256: one more ragged trip of the grid stride
SECOND_TRIP = [((8, 8), torch.float32), ((4, 2), torch.float64)]
LEVELS = (10.0, 1e3)
LEVEL_SHAPES = [(4, 2), (8, 3)]
LADDER = (0.1, 1e-2, 1e-3)
LADDER_SHAPES = [(4, 2), (8, 3), (4, 4), (8, 8)]


def every_shape():
    return [case(d, o, 65, 3, 3) for d, o in ALL_SHAPES]


def edge_cases():
    return [case(d, o, n, b, rows) for d, o in EDGE_SHAPES for n in EDGE_N for b, rows in EDGE_B_ROWS]


def level_cases():
    return [case(d, o, 65, 3, 3, level=lv) for d, o in LEVEL_SHAPES for lv in LEVELS]


def ladder_cases():
    return [case(d, o, 65, 3, 3, ratio=r) for d, o in LADDER_SHAPES for r in LADDER]


def second_trip_case(d, o):
    return case(d, o, SECOND_TRIP_N, 1, 1)


def float32_cases():
    """Every case run in float32: all but the conditioning ladder."""
    return every_shape() + edge_cases() + level_cases()


def benign_cases():
    return every_shape()


# ---------------------------------------------------------------------------------------------------------- running the kernels
def kernel_kind(d, o):
    from pyfilter_amd import _lib as L
    from pyfilter_amd.timeseries import KernelKind

    kind = KernelKind(L.HID_LINEAR_MAT, d, 1.0, 1.0)
    kind.obs_kind, kind.obs_dim = L.OBS_LINEAR, o
    return kind


def device_inputs(c, dtype):
    """``(rows (B, NP), x (D, B, N), z (D, B, N), y (y_rows, O))`` on the GPU in ``dtype``."""
    from pyfilter_amd import ops

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()  # noqa: E731
    return t(c.rows).contiguous(), ops.to_soa(t(c.x), True, True), ops.to_soa(t(c.z), True, True), t(c.y).contiguous()


def run_kernel(c, entry, dtype, own_draws=None):
    """One entry point of ``pf_sample_and_weight`` / ``pf_pre_weight`` on case ``c``: ``(x (N, B, D) | None, w (N, B) | None)`` as
    the device tensors of ``dtype`` in the reference's layout.  ``own_draws = (seed, step)``: the kernel's own Philox normals."""
    from pyfilter_amd import _lib as L
    from pyfilter_amd import ops

    rows, x, z, y = device_inputs(c, dtype)
    kind = kernel_kind(c.d, c.o)
    seed, step = own_draws or (0, 0)
    if own_draws:
        z = None
    if entry.startswith("pre_"):
        code = L.PROP_LGO if entry == "pre_lgo" else L.PROP_BOOTSTRAP
        return None, ops.from_cols(ops.pre_weight_soa(kind, rows, code, x, y), True)
    if entry == "propagate":
        xn, w = ops.sample_and_weight_soa(kind, rows, L.PROP_BOOTSTRAP, x, None, z, seed, step, weigh=False)
        assert w is None
        return ops.from_soa(xn, True, True), None
    xn, w = ops.sample_and_weight_soa(kind, rows, L.PROP_LGO if entry == "lgo" else L.PROP_BOOTSTRAP, x, y, z, seed, step)
    return ops.from_soa(xn, True, True), ops.from_cols(w, True)


def measure(c, entry, dtype):
    """The kernel against the oracle: ``{"x": largest err / bound, "w": ..., "x_err", "w_err": largest errors, "x_ref", "w_ref":
    the reference's float32 errors (float32 only)}``; an output that is not finite counts as infinitely far."""
    res = c.oracle(entry)
    tol_x, tol_w = c.bounds(entry, dtype)
    xn, w = run_kernel(c, entry, dtype)
    out = {}
    for name, got, tol in (("x", xn, tol_x), ("w", w, tol_w)):
        if tol is None:
            assert got is None
            continue
        assert got.dtype == dtype and tuple(got.shape) == res[name].shape
        err = np.abs(got.double().cpu().numpy() - res[name])
        err = np.where(np.isfinite(err), err, np.inf)
        out[name], out[name + "_err"] = float((err / tol).max()), float(err.max())
        if dtype == torch.float32:
            out[name + "_ref"] = float(np.abs(c.reference(entry, dtype)[0 if name == "x" else 1] - res[name]).max())
    return out
