"""TEST INFRASTRUCTURE - an exact host oracle of the ``PF_HID_LINEAR_MAT`` model kernels (``csrc/pf_linear.hpp``):
``x' = b + A x + s e`` observed as ``y ~ N(b_o + A_o x, diag(s_o^2))``, ``1 <= D, O <= 8``, under the bootstrap proposal and the
optimal one (``LinearGaussianObservations``), with both first-stage weights of the auxiliary filter.

It restates the OPERATION, not the kernel: the per-filter constants are formed with mpmath at 60 digits from the covariance form

    S = diag(s_o^2) + A_o diag(s^2) A_o^T,   G = diag(s^2) A_o^T S^-1,   C = (I - G A_o) diag(s^2) = L L^T,   S = Ls Ls^T

(the kernel inverts the precision ``P = diag(s^-2) + A_o^T diag(s_o^-2) A_o`` instead), and the per-particle work is the innovation
form ``mu = m + G (y - b_o - A_o m)``, in which nothing cancels at any ratio ``s_o / s``: the transition residual is ``G r + L z``,
never ``x' - m``, and the observation residual of the new particle is ``R r - A_o L z`` with ``R = I - A_o G = diag(s_o^2) S^-1``.
The per-particle arithmetic runs in numpy's extended precision where the platform has one (x86: 64-bit mantissa) and float64
otherwise, and is returned as float64.

Layouts are the reference's: particles ``(N, B, D)``, log-weights ``(N, B)``; parameter rows ``(B, NP)`` as ``include/pf_amd.h`` packs
them, ``[A D*D | b D | s D | A_o O*D | b_o O | s_o O]``; ``y`` is ``(1, O)`` (shared) or ``(B, O)``.

Besides the values every call returns the magnitudes the tests' bounds are made of (``bounds_f64``):

* ``mag_x (N, B, D)``: ``|K||m| + |c| + |L||z|`` with the kernel's documented constants ``K = C diag(s^-2) = I - G A_o`` and
  ``c = G (y - b_o)`` as the oracle evaluates them; bootstrap / propagate-only: ``|m| + |s z|`` with ``|m| = |b| + |A||x|``, the
  magnitude of the mean's terms (a sum of D + 1 products is rounded against its terms, not against its value, which may cancel);
* ``move (N, B, D)``: ``|G||r| + |L||z|``;
* ``A_w (N, B)``: the sum of the absolute values of the terms of ``log w`` - every ``r^2 / 2 s^2``, ``z^2 / 2``, ``log s``, ``log L_dd``
  and ``k log sqrt(2 pi)`` - and, for every residual that enters a square, ``|d log w / d r| rho`` with ``rho`` the sum of the
  absolute values of the residual's OWN terms (``|y - b_o| + |A_o||x|``): a residual is a difference of quantities of the state's
  size, so its rounding is ``eps rho``, not ``eps |r|``;
* ``grad (N, B, D)``: ``|d log p(y|x') / d x'_d| + |d log p(x'|x) / d x'_d|``, the sensitivity of the terms that are evaluated AT the
  new particle (the proposal density is evaluated at ``z``), term by term - their sum is zero for the optimal proposal;
* ``cond_P (B,)``, ``cond_S (B,)``: 2-norm condition numbers of ``P`` and ``S``."""
import functools
import math

import mpmath
import numpy as np

DPS = 60
EPS64 = 2.0 ** -52
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
# the per-particle arithmetic: extended precision where numpy has one
WORK = np.longdouble if np.finfo(np.longdouble).eps < 1e-18 else np.float64


def split_row(row, d, o):
    """``(A (D, D), b, s, A_o (O, D), b_o, s_o)`` of one packed parameter row."""
    row = np.asarray(row, dtype=np.float64)
    assert row.shape == (d * d + 2 * d + o * d + 2 * o,)
    cuts = np.cumsum([d * d, d, d, o * d, o])
    a, b, s, ao, bo, so = np.split(row, cuts)
    return a.reshape(d, d), b, s, ao.reshape(o, d), bo, so


def pack_row(a, b, s, ao, bo, so):
    return np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, b, s, ao, bo, so)])


def _mp(a):
    a = np.atleast_2d(np.asarray(a, dtype=np.float64))
    return mpmath.matrix([[mpmath.mpf(float(v)) for v in r] for r in a])


def _np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)], dtype=np.float64)


def _diag(v):
    return mpmath.diag([mpmath.mpf(float(x)) for x in v])


def _cond2(m):
    ev = mpmath.eigsy(m, eigvals_only=True)
    ev = [ev[i] for i in range(len(ev))]
    assert min(ev) > 0
    return float(max(ev) / min(ev))


@functools.lru_cache(maxsize=4096)
def _constants(row_bytes, d, o):
    """Everything of one filter that does not depend on ``y`` or the particle, exact to 60 digits, rounded once to float64."""
    with mpmath.workdps(DPS):
        a, b, s, ao, bo, so = split_row(np.frombuffer(row_bytes, dtype=np.float64), d, o)
        Ao, s2, so2 = _mp(ao), _diag(s * s), _diag(so * so)
        S = so2 + Ao * s2 * Ao.T
        S = (S + S.T) / 2
        Sinv = S ** -1
        G = s2 * Ao.T * Sinv
        K = mpmath.eye(d) - G * Ao
        Cm = K * s2
        Cm = (Cm + Cm.T) / 2
        Lc, Ls = mpmath.cholesky(Cm), mpmath.cholesky(S)
        R = so2 * Sinv  # = I - A_o G
        sum_log_l = sum(mpmath.log(Lc[i, i]) for i in range(d))
        sum_log_ls = sum(mpmath.log(Ls[i, i]) for i in range(o))
        sum_log_s = sum(mpmath.log(mpmath.mpf(float(v))) for v in s)
        sum_log_so = sum(mpmath.log(mpmath.mpf(float(v))) for v in so)
        # det C = det(diag s^2) det(diag s_o^2) / det S: the two factorisations agree on the log-determinant
        logdet_gap = abs(2 * sum_log_l - (2 * sum_log_s + 2 * sum_log_so - 2 * sum_log_ls))
        assert abs(2 * sum_log_ls - mpmath.log(mpmath.det(S))) < mpmath.mpf(10) ** -40
        P = _diag(1.0 / s) ** 2 + Ao.T * _diag(1.0 / so) ** 2 * Ao
        P = (P + P.T) / 2
        Lsinv = Ls ** -1
        return {
            "A": a, "b": b, "s": s, "Ao": ao, "bo": bo, "so": so,
            "G": _np(G), "K": _np(K), "L": _np(Lc), "Ls": _np(Ls), "R": _np(R), "Sinv": _np(Sinv), "Lsinv": _np(Lsinv),
            "sum_log_l": float(sum_log_l), "sum_log_ls": float(sum_log_ls), "sum_log_s": float(sum_log_s),
            "sum_log_so": float(sum_log_so), "abs_log_l": float(sum(abs(mpmath.log(Lc[i, i])) for i in range(d))),
            "abs_log_ls": float(sum(abs(mpmath.log(Ls[i, i])) for i in range(o))),
            "abs_log_s": float(sum(abs(math.log(v)) for v in s)), "abs_log_so": float(sum(abs(math.log(v)) for v in so)),
            "logdet_gap": float(logdet_gap), "cond_P": _cond2(P), "cond_S": _cond2(S),
        }


def constants(row, d, o):
    return _constants(np.ascontiguousarray(row, dtype=np.float64).tobytes(), d, o)


def _w(a):
    return np.asarray(a, dtype=WORK)


def _rows_of(y, nb):
    y = np.asarray(y, dtype=np.float64)
    assert y.ndim == 2 and y.shape[0] in (1, nb), y.shape
    return [y[0 if y.shape[0] == 1 else k] for k in range(nb)]


def sample_and_weight(rows, y, x, z, d, o, proposal, weigh=True):
    """``proposal``: ``"lgo"`` or ``"bootstrap"``; ``weigh = False`` (``y`` unused): propagate only, from the dynamics.
    Returns a dict of float64 arrays: ``x``, ``w`` (None without weights) and the magnitudes of the module's docstring."""
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    n, nb, _ = x.shape
    lgo = weigh and proposal == "lgo"
    ys = _rows_of(y, nb) if weigh else [None] * nb
    out = {k: np.zeros((n, nb, d)) for k in ("x", "mag_x", "move", "grad")}
    out.update({k: np.zeros((n, nb)) for k in ("w", "A_w")})
    out["cond_P"], out["cond_S"], out["lgo"] = np.zeros(nb), np.zeros(nb), lgo
    for k in range(nb):
        c = constants(rows[k], d, o)
        out["cond_P"][k], out["cond_S"][k] = c["cond_P"], c["cond_S"]
        A, b, s, Ao, bo, so = (_w(c[q]) for q in ("A", "b", "s", "Ao", "bo", "so"))
        xk, zk = _w(x[:, k]), _w(z[:, k])
        m = b + xk @ A.T
        if not lgo:
            step = s * zk
            xn = m + step
            out["mag_x"][:, k] = np.abs(b) + np.abs(xk) @ np.abs(A).T + np.abs(step)
            out["move"][:, k] = np.abs(step)
            robs_own = None
        else:
            G, Lc, R = _w(c["G"]), _w(c["L"]), _w(c["R"])
            yb = _w(ys[k]) - bo
            r = yb - m @ Ao.T
            gr, lz = r @ G.T, zk @ Lc.T
            xn = (m + gr) + lz
            out["mag_x"][:, k] = np.abs(m) @ np.abs(_w(c["K"])).T + np.abs(yb @ G.T) + np.abs(zk) @ np.abs(Lc).T
            out["move"][:, k] = np.abs(r) @ np.abs(G).T + np.abs(zk) @ np.abs(Lc).T
            robs_own = r @ R.T - lz @ Ao.T  # y - b_o - A_o x', without the cancellation
            dx = gr + lz                    # x' - m, likewise
        out["x"][:, k] = xn
        if not weigh:
            continue
        yb = _w(ys[k]) - bo
        robs = robs_own if lgo else yb - xn @ Ao.T
        rho = np.abs(yb) + np.abs(xn) @ np.abs(Ao).T
        lw = -(robs * robs / (2 * so * so)).sum(-1) - WORK(c["sum_log_so"]) - o * WORK(LOG_SQRT_2PI)
        a_w = (robs * robs / (2 * so * so)).sum(-1) + c["abs_log_so"] + o * LOG_SQRT_2PI + (np.abs(robs) / (so * so) * rho).sum(-1)
        grad = np.abs((robs / (so * so)) @ Ao)
        if lgo:
            e = dx / s
            lw = lw - (e * e).sum(-1) / 2 - WORK(c["sum_log_s"]) + (zk * zk).sum(-1) / 2 + WORK(c["sum_log_l"])
            a_w = a_w + (e * e).sum(-1) / 2 + c["abs_log_s"] + (zk * zk).sum(-1) / 2 + c["abs_log_l"] + 2 * d * LOG_SQRT_2PI
            grad = grad + np.abs(dx) / (s * s)
        out["w"][:, k], out["A_w"][:, k], out["grad"][:, k] = lw, a_w, grad
    if not weigh:
        out["w"] = out["A_w"] = None
    return out


def pre_weight(rows, y, x, d, o, proposal):
    """Bootstrap: ``log p(y | b + A x)``; LGO: ``log N(y; b_o + A_o x, S)`` at the UN-propagated particle.  ``w``, ``A_w (N, B)``."""
    x = np.asarray(x, dtype=np.float64)
    n, nb, _ = x.shape
    ys = _rows_of(y, nb)
    out = {"w": np.zeros((n, nb)), "A_w": np.zeros((n, nb)), "cond_P": np.zeros(nb), "cond_S": np.zeros(nb), "solve": proposal == "lgo"}
    for k in range(nb):
        c = constants(rows[k], d, o)
        out["cond_P"][k], out["cond_S"][k] = c["cond_P"], c["cond_S"]
        A, b, Ao, bo, so = (_w(c[q]) for q in ("A", "b", "Ao", "bo", "so"))
        xk = _w(x[:, k])
        yb = _w(ys[k]) - bo
        if proposal != "lgo":
            r = yb - (b + xk @ A.T) @ Ao.T
            rho = np.abs(yb) + (np.abs(b) + np.abs(xk) @ np.abs(A).T) @ np.abs(Ao).T
            q = (r * r / (2 * so * so)).sum(-1)
            out["w"][:, k] = -q - WORK(c["sum_log_so"]) - o * WORK(LOG_SQRT_2PI)
            out["A_w"][:, k] = q + c["abs_log_so"] + o * LOG_SQRT_2PI + (np.abs(r) / (so * so) * rho).sum(-1)
        else:
            r = yb - xk @ Ao.T
            rho = np.abs(yb) + np.abs(xk) @ np.abs(Ao).T
            t = r @ _w(c["Lsinv"]).T  # whitened innovation
            q = (t * t).sum(-1) / 2
            out["w"][:, k] = -q - WORK(c["sum_log_ls"]) - o * WORK(LOG_SQRT_2PI)
            out["A_w"][:, k] = q + c["abs_log_ls"] + o * LOG_SQRT_2PI + (np.abs(r @ _w(c["Sinv"]).T) * rho).sum(-1)
    return out


# ---------------------------------------------------------------------------------------------------------------- the bounds
def bounds_f64(res, d):
    """``(tol_x (N, B, D) | None, tol_w (N, B) | None)`` of a float64 kernel against a ``sample_and_weight`` / ``pre_weight``
    result of this module (eps = 2^-52):

        tol_x = 16 eps cond_2(P) (|K||m| + |c| + |L||z|) + 4 eps |x'|          (bootstrap, propagate-only: 4 eps (|m| + |s z|))
        tol_w = sum_d |d log w / d x'_d| tol_x_d + 16 eps A_w + 4 D eps cond_2(P)
        pre-weight: 16 eps A_w + 4 D eps cond_2(S)                               (the bootstrap one solves nothing: 16 eps A_w)

    The kernel forms ``C = P^-1`` through a Cholesky factor of ``P`` in double: relative error about ``cond(P) eps`` in ``K``, ``c``
    and ``L``, which multiply ``m``, 1 and ``z``; 16 covers the up to 8-term products and the two triangular solves.  Everything else
    is a sum of at most 17 products of the arithmetic type."""
    tol_x = tol_w = None
    if "x" in res:
        if res["lgo"]:
            tol_x = 16 * EPS64 * res["cond_P"][None, :, None] * res["mag_x"] + 4 * EPS64 * np.abs(res["x"])
        else:
            tol_x = 4 * EPS64 * res["mag_x"]
        if res["w"] is not None:
            solve = 4 * d * EPS64 * res["cond_P"][None, :] if res["lgo"] else 0.0
            tol_w = (res["grad"] * tol_x).sum(-1) + 16 * EPS64 * res["A_w"] + solve
    else:
        tol_w = 16 * EPS64 * res["A_w"] + (4 * d * EPS64 * res["cond_S"][None, :] if res.get("solve") else 0.0)
    return tol_x, tol_w
