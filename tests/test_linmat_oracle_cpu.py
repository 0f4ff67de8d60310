"""The exact oracle of the ``PF_HID_LINEAR_MAT`` kernels (``tests/linmat_oracle.py``) and the conditions its case list
(``tests/linmat_cases.py``) has to meet before the GPU parity test (``tests/test_linmat_parity_gpu.py``) means anything.  No GPU."""
import numpy as np
import pytest
import torch

from tests import linear_cases as FX
from tests import linmat_cases as LC
from tests import linmat_oracle as LO


def _rel(got, ref):
    return float((np.abs(got - ref) / (1.0 + np.abs(ref))).max())


@pytest.mark.parametrize("d", range(1, 9))
def test_oracle_agrees_with_the_reference_arithmetic_in_float64(d):
    """At the benign regime (s_o / s = 2, states of O(1)) torch float64 evaluates the reference's formulas - the precision form, a
    matrix inverse per particle - to within 1e-12 of the oracle's covariance form: two derivations of one operation."""
    for c in LC.every_shape():
        if c.d != d:
            continue
        for entry in LC.ENTRY_POINTS:
            res, (rx, rw) = c.oracle(entry), c.reference(entry, torch.float64)
            if rx is not None:
                assert _rel(rx, res["x"]) <= 1e-12, (c, entry)
            if rw is not None:
                assert _rel(rw, res["w"]) <= 1e-12, (c, entry)


@pytest.mark.parametrize("name", list(FX.CASES))
def test_oracle_reproduces_the_reference_fixtures_teacher_forced(name):
    """Move by move from the reference's own recorded state (resampled with its recorded ancestors) the oracle gives the reference's
    particles and log-weights at 1e-9: the fixtures are the unmodified reference's numbers."""
    g = {k: v.double() if v.is_floating_point() else v for k, v in FX.load(name, "f64").items()}
    filt_name, prop, ess, _ = FX.CASES[name]
    (n, b, d), o = g["x0"].shape, g["obs_A"].shape[0]
    shapes = {"hid_A": (d, d), "hid_b": (d,), "hid_s": (d,), "obs_A": (o, d), "obs_b": (o,), "obs_s": (o,)}
    per_filter = {k: np.broadcast_to(g[k].numpy(), (b,) + s) for k, s in shapes.items()}  # (a parameter may carry the batch dim)
    rows = np.stack([LO.pack_row(*(per_filter[k][i] for k in shapes)) for i in range(b)])
    tol = dict(rtol=1e-9, atol=1e-9)
    x, w = g["x0"], torch.zeros(n, b, dtype=torch.float64)
    for t in range(g["y"].shape[0]):
        y, idx = g["y"][t].numpy()[None], g["step_idx"][t]
        xg = x.gather(0, idx.unsqueeze(-1).expand_as(x))
        if filt_name == "sisr":
            W = torch.softmax(w, 0)
            mask = 1.0 / W.square().sum(0) < ess * n
            xr, wr = torch.where(mask.view(1, b, 1), xg, x), torch.where(mask.view(1, b), torch.zeros_like(w), w)
        else:
            xr = xg
        observed = not np.isnan(y).all()
        res = LO.sample_and_weight(rows, y, xr.numpy(), g["z_tape"][t].numpy(), d, o, prop, weigh=observed)
        torch.testing.assert_close(torch.from_numpy(res["x"]), g["step_x"][t], rtol=1e-9, atol=1e-11)
        if not observed:
            w_new = wr
        elif filt_name == "sisr":
            w_new = torch.from_numpy(res["w"]) + wr
        else:
            pre = torch.from_numpy(LO.pre_weight(rows, y, x.numpy(), d, o, prop)["w"])
            w_new = torch.from_numpy(res["w"]) - pre.gather(0, idx)
        torch.testing.assert_close(w_new, g["step_w"][t], **tol)
        x, w = g["step_x"][t], g["step_w"][t]


def test_the_two_factorisations_agree_on_the_log_determinant():
    """``2 sum log diag chol(C) = log det(diag s^2) + log det(diag s_o^2) - log det S`` to 50 digits, at every shape and ratio."""
    for c in LC.every_shape() + LC.ladder_cases() + LC.level_cases():
        for row in c.rows:
            k = LO.constants(row, c.d, c.o)
            assert k["logdet_gap"] < 1e-50, (c, k["logdet_gap"])
            # ... and in float64 the kernel's constant k_q - k_trans = sum log L_dd - sum log s_d is what the oracle subtracts
            assert abs(k["sum_log_l"] - (k["sum_log_s"] + k["sum_log_so"] - k["sum_log_ls"])) <= 1e-14 * (1 + k["abs_log_l"] + k["abs_log_ls"])


def test_no_case_is_conditioned_beyond_the_cap():
    """``cond_2(P) <= 1e8`` in every case: beyond it the float64 bound ``16 eps cond(P)`` exceeds 1e-7 of the particle and tests nothing."""
    conds = {repr(c): c.cond_P() for c in LC.every_shape() + LC.edge_cases() + LC.level_cases() + LC.ladder_cases()}
    conds.update({repr(c): c.cond_P() for c in (LC.second_trip_case(d, o) for (d, o), _ in LC.SECOND_TRIP)})
    assert max(conds.values()) <= LC.COND_CAP, max(conds, key=conds.get)
    # the benign regime is benign: the float64 bound there is ~1e-13 of a particle, no wrong index or sign passes it
    assert max(c.cond_P() for c in LC.every_shape()) <= 1e3
    # ... and the ladder does climb
    assert max(c.cond_P() for c in LC.ladder_cases()) >= 1e6


def test_the_reference_completes_every_float32_case():
    """Its own float32 arithmetic factorises a positive-definite covariance and returns finite numbers: the float32 bound, measured
    from it, exists."""
    cases = LC.float32_cases() + [LC.second_trip_case(d, o) for (d, o), dt in LC.SECOND_TRIP if dt == torch.float32]
    for c in cases:
        assert c.reference_completes_in_float32(), c


def _moved_rows(c):
    """The case with filter 0's observation row / parameter row handed to every filter."""
    same_y = LC.Case(c.d, c.o, c.n, c.b, c.y_rows, c.ratio, c.level, c.seed)
    same_y.y = np.stack([c.y[0]] * c.y_rows)
    same_row = LC.Case(c.d, c.o, c.n, c.b, c.y_rows, c.ratio, c.level, c.seed)
    same_row.rows = np.stack([c.rows[0]] * c.b)
    return same_y, same_row


@pytest.mark.parametrize("shape", LC.EDGE_SHAPES, ids=str)
def test_rows_differ_by_more_than_a_thousand_bounds(shape):
    """A kernel that read observation row 0, or parameter row 0, for every filter is off by more than 1e3 x the bound, in both
    dtypes, at every entry point that reads the row."""
    c = LC.case(*shape, 65, 3, 3)
    same_y, same_row = _moved_rows(c)
    for dtype in (torch.float64, torch.float32):
        for entry in LC.ENTRY_POINTS:
            res = c.oracle(entry)
            tol_x, tol_w = c.bounds(entry, dtype)
            for other, reads in ((same_y, entry != "propagate"), (same_row, True)):
                if not reads:
                    continue
                wrong = other.oracle(entry)
                for k in (1, 2):
                    if tol_w is not None:
                        gap, tol = np.abs(wrong["w"] - res["w"])[:, k], np.broadcast_to(tol_w, res["w"].shape)[:, k]
                        assert gap.max() > 1e3 * tol.max(), (c, entry, dtype, k)
                    if tol_x is not None and (other is same_row or entry == "lgo"):  # (a bootstrap move does not read y)
                        gap, tol = np.abs(wrong["x"] - res["x"])[:, k], np.broadcast_to(tol_x, res["x"].shape)[:, k]
                        assert gap.max() > 1e3 * tol.max(), (c, entry, dtype, k)


def test_no_bound_is_zero_where_a_term_exists():
    for c in LC.every_shape() + LC.ladder_cases() + LC.level_cases() + [LC.case(4, 2, 1, 1, 1), LC.case(7, 1, 257, 3, 3)]:
        for dtype in (torch.float64, torch.float32) if c.ratio == 2.0 else (torch.float64,):  # (the ladder is float64 only)
            for entry in LC.ENTRY_POINTS:
                res = c.oracle(entry)
                tol_x, tol_w = c.bounds(entry, dtype)
                assert (tol_x is None) == ("x" not in res) and (tol_w is None) == (res["w"] is None)
                if tol_x is not None:
                    assert np.isfinite(tol_x).all() and (tol_x > 0).all() and (tol_x < 1e-3 * (1 + np.abs(res["x"]))).all(), (c, entry)
                if tol_w is not None:
                    assert np.isfinite(tol_w).all() and (tol_w > 0).all(), (c, entry)
