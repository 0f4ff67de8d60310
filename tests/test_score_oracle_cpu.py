"""The path-score oracle (``tests/score_oracle.py``) and the host side of ``ParticleFilter.path_score``, without a GPU:

* the oracle's gradient against central finite differences of its own value, every kind and shape of row;
* ``path_score(route="torch")`` on CPU tensors - the package's own densities under torch autograd - equals the oracle plus the
  initial term, value and gradient, so the oracle restates what the package's model classes define;
* the kernel route's step from row gradients to named parameters (the vector-Jacobian product through the model builder and
  ``pack_params``), with the kernel replaced by the oracle: a per-filter parameter, a shared scalar, a transformed parameter,
  Lorenz-63's component-0 slots;
* the entry points are declared (header, ``_lib.EXPORTS``, ABI 4) and refuse what they do not implement before any launch."""
import ctypes as C
import os

import pytest
import torch

from pyfilter_amd import _lib as L
from pyfilter_amd import timeseries as ts
from pyfilter_amd.filters.particle import SISR
from pyfilter_amd.filters.particle import score as score_mod
from pyfilter_amd.timeseries import models
from tests import score_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.fixture(autouse=True)
def float64_models():
    """Models built here hold float64 constants (the increment scale sqrt(dt) of the Euler-Maruyama kinds among them)."""
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(before)


ALL_KINDS = [so.Kind(name, d, o, sv) for name in ("linear", "sine", "verhulst", "ou") for d, o, sv in
             ((1, 1, False), (1, 1, True), (2, 1, False), (2, 2, False), (3, 1, False), (3, 3, False))]
ALL_KINDS += [so.Kind("lorenz", 3, 1), so.Kind("lorenz", 3, 3)]


@pytest.mark.parametrize("kind", ALL_KINDS, ids=repr)
def test_oracle_gradient_is_the_derivative_of_its_value(kind):
    inp = so.Inputs(kind, 4, 5, 2, by=2, seed=1)
    ref = so.score(kind, inp.rows, inp.paths, inp.y)
    value = lambda rows: so.score(kind, rows, inp.paths, inp.y, per_term=False)["value"]  # noqa: E731
    torch.testing.assert_close(value(inp.rows), ref["value"], rtol=1e-13, atol=0.0)
    for k in range(kind.n_params):
        h = 1e-6 * inp.rows[:, k].abs().clamp_min(1.0)
        step = torch.zeros_like(inp.rows)
        step[:, k] = h
        fd = (value(inp.rows + step) - value(inp.rows - step)) / (2.0 * h)
        bound = 1e-6 * ref["A_grad"][:, k] + 1e-7 * ref["A_value"] * (ref["A_grad"][:, k] > 0)
        assert bool(((fd - ref["grad"][:, k]).abs() <= bound).all()), (kind, k, fd, ref["grad"][:, k], bound)


def test_oracle_skips_unobserved_rows_and_poisons_half_observed_ones():
    kind = so.Kind("lorenz", 3, 3)
    inp = so.Inputs(kind, 5, 6, 3, by=3, seed=2)
    y = inp.y.clone()
    y[1] = float("nan")           # nobody observes state 2
    y[2, 1, 0] = float("nan")     # filter 1 observes state 3 in part
    got = so.score(kind, inp.rows, inp.paths, y)
    assert got["value"][1].isnan() and got["grad"][1].isnan().all()
    keep = torch.tensor([0, 2])
    # the fully observed sums less the observation term of row 1 (transition 1 -> 2 with and without its observation)
    full = so.score(kind, inp.rows, inp.paths, inp.y)
    only = so.score(kind, inp.rows, inp.paths[1:3], inp.y[1:2])          # transition 1 -> 2 and its observation
    trans = so.score(kind, inp.rows, inp.paths[1:3], torch.full_like(inp.y[1:2], float("nan")))  # that transition alone
    expect = full["value"] - (only["value"] - trans["value"])
    torch.testing.assert_close(got["value"][keep], expect[keep], rtol=1e-12, atol=1e-12)


# ----------------------------------------------------------------------------------------------------------------
# the package's model classes from a parameter row
# ----------------------------------------------------------------------------------------------------------------
def model_from_rows(kind, rows):
    d, o = kind.dim, kind.obs_dim
    hp = [rows[:, k * d:(k + 1) * d] for k in range(4)]
    col = lambda t: t[:, 0]  # noqa: E731
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    if kind.name == "linear":
        hidden = models.AR(col(hp[0]), col(hp[1]), col(hp[2]))
    elif kind.name == "sine":
        hidden = models.SineDiffusion(col(hp[0]), col(hp[1]), dt=kind.dt, initial=(f64(3.6), f64(1.0)))
    elif kind.name == "verhulst":
        hidden = models.Verhulst(col(hp[0]), col(hp[1]), col(hp[2]), dt=kind.dt)
    elif kind.name == "ou":
        hidden = models.OrnsteinUhlenbeck(col(hp[0]), col(hp[1]), col(hp[2]), dt=kind.dt)
    else:
        hidden = models.Lorenz63(hp[0][:, 0], hp[1][:, 0], hp[2][:, 0], hp[3], dt=kind.dt,
                                 initial_mean=f64([-5.9, -5.5, 24.5]), initial_scale=f64([3.0, 3.0, 3.0]))
    a = rows[:, 4 * d:4 * d + o * d]
    ob, os_ = rows[:, 4 * d + o * d:4 * d + o * d + o], rows[:, 4 * d + o * d + o:]
    if kind.obs_kind == L.OBS_SV:
        return models.StochasticVolatilityModel(hidden, col(ob))
    if d == 1:
        return ts.LinearStateSpaceModel(hidden, (col(a), col(ob), col(os_)))
    return ts.LinearStateSpaceModel(hidden, (a.reshape(-1, o, d), ob, os_), event_shape=torch.Size([o]))


def reference_layout(kind, paths, y):
    """Oracle layouts -> ``paths (S, N, B, [D])``, ``y (S-1, [By], [O])`` as the filter's users hold them."""
    p = paths if kind.dim > 1 else paths[..., 0]
    yy = y if kind.obs_dim > 1 or kind.dim > 1 else y[..., 0]
    return p, (yy[:, 0] if y.shape[1] == 1 else yy)


TORCH_KINDS = [so.Kind("linear", 1, 1), so.Kind("linear", 1, 1, True), so.Kind("sine", 1, 1), so.Kind("sine", 1, 1, True),
               so.Kind("verhulst", 1, 1), so.Kind("verhulst", 1, 1, True), so.Kind("ou", 1, 1), so.Kind("ou", 1, 1, True),
               so.Kind("lorenz", 3, 3)]


def _filter(kind, b, n=8):
    filt = SISR(lambda theta: model_from_rows(kind, theta["rows"]), n)
    filt.set_batch_shape(torch.Size([b]))
    return filt


def _initial_term(kind, rows, paths):
    leaf = rows.clone().requires_grad_(True)
    init = model_from_rows(kind, leaf).hidden.initial_distribution.log_prob(paths[0]).mean(0)
    if init.requires_grad:  # (a fixed initial law depends on no parameter)
        init.sum().backward()
    return init.detach(), (leaf.grad if leaf.grad is not None else torch.zeros_like(rows))


@pytest.mark.parametrize("by", (1, 3))
@pytest.mark.parametrize("kind", TORCH_KINDS, ids=repr)
def test_torch_route_on_cpu_equals_the_oracle(kind, by):
    b = 3
    inp = so.Inputs(kind, 6, 8, b, by=by, seed=3)
    y = inp.y.clone()
    y[2] = float("nan")  # (skipped on both sides)
    ref = so.score(kind, inp.rows, inp.paths, y)
    paths, yy = reference_layout(kind, inp.paths, y)
    assert kind.dim > 1 or kind.obs_dim == 1
    filt = _filter(kind, b)
    theta = {"rows": inp.rows}
    filt.initialize_model(theta)
    assert so.Kind.of(filt.ssm.kernel_kind).n_params == kind.n_params
    init, init_grad = _initial_term(kind, inp.rows, paths)
    value = filt.path_score(paths, yy, route="torch")
    torch.testing.assert_close(value, ref["value"] + init, rtol=1e-12, atol=1e-12)
    value2, grads = filt.path_score(paths, yy, theta=theta, route="torch")
    torch.testing.assert_close(value2, value, rtol=0, atol=0)
    err = (grads["rows"] - (ref["grad"] + init_grad)).abs()
    assert bool((err <= 1e-10 * (ref["A_grad"] + init_grad.abs())).all()), err.max()
    assert filt.path_score(paths, yy, route="auto").equal(value)  # (CPU tensors: the torch route)
    with pytest.raises(L.PfAmdError):
        filt.path_score(paths, yy, route="kernel")


def test_half_observed_rows_are_nan_for_their_filters_on_the_torch_route():
    kind, b = so.Kind("lorenz", 3, 3), 3
    inp = so.Inputs(kind, 5, 6, b, by=b, seed=4)
    y = inp.y.clone()
    y[1, 2, 1] = float("nan")
    filt = _filter(kind, b)
    filt.initialize_model({"rows": inp.rows})
    value, grads = filt.path_score(inp.paths, y, theta={"rows": inp.rows}, route="torch")
    assert value.isnan().tolist() == [False, False, True]
    assert grads["rows"][2].isnan().all() and torch.isfinite(grads["rows"][:2]).all()


def test_observe_every_step_other_than_one_is_refused():
    hidden = models.AR(0.1, 0.9, 0.3)
    filt = SISR(ts.LinearStateSpaceModel(hidden, (1.0, 0.5), observe_every_step=2), 8)
    with pytest.raises(NotImplementedError):
        filt.path_score(torch.zeros(3, 8, dtype=torch.float64), torch.zeros(2, dtype=torch.float64))


# ----------------------------------------------------------------------------------------------------------------
# rows -> names: the kernel route with the kernel replaced by the oracle
# ----------------------------------------------------------------------------------------------------------------
def _oracle_in_place_of_the_kernel(monkeypatch):
    def fake(kind, params, soa, y):
        s, d, b, n = soa.shape
        got = so.score(so.Kind.of(kind), params.double(), soa.permute(0, 3, 2, 1).double(), y.double().reshape(s - 1, -1, kind.obs_dim))
        return got["value"], got["grad"]

    monkeypatch.setattr(score_mod, "kernel_applies", lambda model, paths: True)
    monkeypatch.setattr(score_mod.ops, "path_score", fake)


def _builders():
    t = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731

    def ar(theta):       # a per-filter (B,) parameter and a shared scalar
        return ts.LinearStateSpaceModel(models.AR(t(0.1), theta["beta"], theta["sigma"]), (t(1.0), t(0.1), theta["s"]))

    def ou(theta):       # a transformed parameter: the builder takes the square root of a variance
        return ts.LinearStateSpaceModel(models.OrnsteinUhlenbeck(theta["kappa"], t(1.0), theta["v"].sqrt()), (t(0.7), t(0.5)))

    def lorenz(theta):   # s, r, b land in component 0 of hp0 .. hp2, sigma in hp3
        hidden = models.Lorenz63(theta["s"], theta["r"], t(8.0 / 3.0), theta["sigma"], initial_mean=t([-5.9, -5.5, 24.5]),
                                 initial_scale=t([3.0, 3.0, 3.0]))
        return ts.LinearStateSpaceModel(hidden, (torch.eye(3, dtype=torch.float64), theta["s_obs"]), event_shape=torch.Size([3]))

    b = 2  # (not the state dimension: a (3,) parameter of a three-component state is read per component)
    per = lambda lo, hi: torch.linspace(lo, hi, b, dtype=torch.float64)  # noqa: E731
    return {
        "ar": (so.Kind("linear", 1, 1), ar, {"beta": per(0.85, 0.95), "sigma": t(0.3), "s": per(0.4, 0.6)}),
        "ou": (so.Kind("ou", 1, 1), ou, {"kappa": per(0.4, 0.6), "v": t(0.16)}),
        "lorenz": (so.Kind("lorenz", 3, 3), lorenz, {"s": per(9.5, 10.5), "r": t(28.0), "sigma": t([1.0, 1.2, 0.8]),
                                                     "s_obs": per(0.4, 0.6).unsqueeze(-1).expand(b, 3).contiguous()}),
    }


@pytest.mark.parametrize("name", ("ar", "ou", "lorenz"))
def test_row_gradients_reach_the_named_parameters(name, monkeypatch):
    kind, builder, theta = _builders()[name]
    b = 2
    inp = so.Inputs(kind, 6, 8, b, by=1, seed=5)
    paths, y = reference_layout(kind, inp.paths, inp.y)
    filt = SISR(builder, 8)
    filt.set_batch_shape(torch.Size([b]))
    filt.initialize_model(theta)
    want_value, want = filt.path_score(paths, y, theta=theta, route="torch")
    _oracle_in_place_of_the_kernel(monkeypatch)
    value, got = filt.path_score(paths, y, theta=theta, route="kernel")
    torch.testing.assert_close(value, want_value, rtol=1e-12, atol=1e-12)
    assert set(got) == set(theta)
    for k in theta:
        assert got[k].shape == theta[k].shape, k
        torch.testing.assert_close(got[k], want[k], rtol=1e-9, atol=1e-9, msg=k)
        assert not theta[k].requires_grad  # (the caller's tensors are cloned, not touched)
    without = filt.path_score(paths, y, route="kernel")
    torch.testing.assert_close(without, value, rtol=0, atol=0)


# ----------------------------------------------------------------------------------------------------------------
# the C ABI
# ----------------------------------------------------------------------------------------------------------------
def test_entry_points_declared():
    assert "pf_path_score" in L.EXPORTS and "pf_path_score_workspace_bytes" in L.EXPORTS
    assert L.ABI_VERSION == 4
    with open(os.path.join(ROOT, "include", "pf_amd.h")) as f:
        header = f.read()
    assert "int pf_path_score(const pf_model* model, const void* paths, const void* y, int64_t y_rows, double* value, double* grad," in header
    assert "int pf_path_score_workspace_bytes(int64_t N, int64_t B, int64_t S, size_t* bytes);" in header
    assert "gradient.py:9-32" in header and "#define PF_ABI_VERSION 4" in header
    lib = L.load()
    assert lib.pf_abi_version() == 4 and hasattr(lib, "pf_path_score") and hasattr(lib, "pf_path_score_workspace_bytes")


def test_refusals_come_before_any_launch():
    lib = L.load()
    n = C.c_size_t(0)
    assert lib.pf_path_score_workspace_bytes(1024, 3, 17, C.byref(n)) == 0 and n.value > 0
    assert lib.pf_path_score_workspace_bytes(1024, 3, 1, C.byref(n)) == -1   # S < 2: PF_EINVAL
    assert lib.pf_path_score_workspace_bytes(0, 3, 17, C.byref(n)) == -1

    def call(hid, d, o, s=5, rows=1, obs=L.OBS_LINEAR, ws=1 << 20):
        m = L.PfModel()
        m.hid_kind, m.obs_kind, m.dim, m.obs_dim, m.dt, m.inc_scale, m.params = hid, obs, d, o, 1.0, 1.0, 8
        return lib.pf_path_score(C.byref(m), 8, 8, rows, 8, 8, 8, ws, s, 64, 2, L.PF_F64, None)

    assert call(L.HID_LINEAR_MAT, 2, 2) == -3      # PF_EUNSUPPORTED
    assert call(L.HID_USER_AFFINE, 1, 1) == -3
    assert call(L.HID_LINEAR, 4, 1) == -3          # D, O above 3
    assert call(L.HID_LINEAR, 2, 4) == -3
    assert call(L.HID_LORENZ63_EM, 2, 1) == -3
    assert call(L.HID_SINE_EM, 2, 1, obs=L.OBS_SV) == -3
    assert call(L.HID_LINEAR, 1, 1, s=1) == -1     # PF_EINVAL
    assert call(L.HID_LINEAR, 1, 1, rows=3) == -1  # neither 1 nor B
    assert call(L.HID_LINEAR, 1, 1, ws=8) == -2    # PF_EWORKSPACE
    m = L.PfModel()
    assert lib.pf_path_score(C.byref(m), 8, 8, 1, 8, 8, 8, 1 << 20, 5, 64, 2, L.PF_F64, None) == -1  # no parameter rows
