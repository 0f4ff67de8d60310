"""The oracle of the ``pf_path_score_linear`` tests (``tests/linmat_score_oracle.py``) pinned, without a GPU, to what the package's
model classes define: ``path_score(route="torch")`` on CPU tensors - ``LinearModel``'s and ``LinearStateSpaceModel``'s own
``log_prob``s under torch autograd - equals the oracle plus the initial term, value and gradient, to the tolerance
``tests/test_score_oracle_cpu.py`` uses for the same comparison of the built-in kinds (1e-12 on the value, ``1e-10 A`` per
gradient slot); and the oracle's gradient is the derivative of its value, its NaN conventions are ``pf_path_score``'s."""
import pytest
import torch
from torch.distributions import Independent, Normal

from pyfilter_amd import _lib as L
from pyfilter_amd import timeseries as ts
from pyfilter_amd.filters.particle import SISR
from pyfilter_amd.timeseries import models
from tests import linmat_score_oracle as lso

SHAPES = ((1, 1), (2, 3), (4, 2), (8, 8))


def model_from_rows(d, o, rows):
    a, off, s, ao, bo, so = lso.split(rows, d, o)
    m0, s0 = torch.ones(d, dtype=torch.float64), 0.5 * torch.ones(d, dtype=torch.float64)
    inc = Independent(Normal(torch.tensor(0.0, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64)).expand(torch.Size([d])), 1)
    hidden = models.LinearModel((a, off, s), inc, lambda *_: Independent(Normal(m0, s0), 1))
    return ts.LinearStateSpaceModel(hidden, (ao, bo, so), torch.Size([o]))


def _filter(d, o, b, n):
    filt = SISR(lambda theta: model_from_rows(d, o, theta["rows"]), n)
    filt.set_batch_shape(torch.Size([b]))
    return filt


@pytest.mark.parametrize("by", (1, 3))
@pytest.mark.parametrize("d,o", SHAPES)
def test_torch_route_on_cpu_equals_the_oracle(d, o, by):
    b, n = 3, 8
    inp = lso.Inputs(d, o, 6, n, b, by=by, seed=3)
    y = inp.y.clone()
    y[2] = float("nan")  # (skipped on both sides)
    ref = lso.score(d, o, inp.rows, inp.paths, y)
    yy = y[:, 0] if by == 1 else y
    filt = _filter(d, o, b, n)
    theta = {"rows": inp.rows}
    filt.initialize_model(theta)
    kind = filt.ssm.kernel_kind
    assert kind.hid_kind == L.HID_LINEAR_MAT and (kind.dim, kind.obs_dim) == (d, o)
    init = filt.ssm.hidden.initial_distribution.log_prob(inp.paths[0]).mean(0)  # (a fixed initial law: no gradient)
    value = filt.path_score(inp.paths, yy, route="torch")
    torch.testing.assert_close(value, ref["value"] + init, rtol=1e-12, atol=1e-12)
    value2, grads = filt.path_score(inp.paths, yy, theta=theta, route="torch")
    torch.testing.assert_close(value2, value, rtol=0, atol=0)
    err = (grads["rows"] - ref["grad"]).abs()
    assert bool((err <= 1e-10 * ref["A_grad"]).all()), (err / ref["A_grad"]).max()
    assert bool((ref["A_grad"] > 0).all())  # (every slot of the row is read)
    assert filt.path_score(inp.paths, yy, route="auto").equal(value)  # (CPU tensors: the torch route)
    with pytest.raises(L.PfAmdError):
        filt.path_score(inp.paths, yy, route="kernel")


def test_oracle_gradient_is_the_derivative_of_its_value():
    d, o = 3, 2
    inp = lso.Inputs(d, o, 5, 6, 2, seed=1)
    ref = lso.score(d, o, inp.rows, inp.paths, inp.y)
    plain = lso.score(d, o, inp.rows, inp.paths, inp.y, per_term=False)
    torch.testing.assert_close(plain["grad"], ref["grad"], rtol=1e-12, atol=1e-12)
    h = 1e-6
    for k in range(lso.n_params(d, o)):
        up, dn = inp.rows.clone(), inp.rows.clone()
        up[:, k] += h
        dn[:, k] -= h
        fd = (lso.score(d, o, up, inp.paths, inp.y, per_term=False)["value"]
              - lso.score(d, o, dn, inp.paths, inp.y, per_term=False)["value"]) / (2 * h)
        assert bool(((fd - ref["grad"][:, k]).abs() <= 1e-6 * ref["A_grad"][:, k] + 1e-7).all()), k


def test_oracle_skips_unobserved_rows_and_poisons_half_observed_ones():
    d, o, b = 2, 2, 3
    inp = lso.Inputs(d, o, 6, 5, b, by=b, seed=2)
    full = lso.score(d, o, inp.rows, inp.paths, inp.y)
    y = inp.y.clone()
    y[1] = float("nan")
    skipped = lso.score(d, o, inp.rows, inp.paths, y)
    assert torch.isfinite(skipped["value"]).all() and not torch.equal(skipped["value"], full["value"])
    y[3, 2, 0] = float("nan")
    got = lso.score(d, o, inp.rows, inp.paths, y)
    assert got["value"].isnan().tolist() == [False, False, True] and got["grad"][2].isnan().all()
    torch.testing.assert_close(got["value"][:2], skipped["value"][:2], rtol=1e-12, atol=1e-12)
