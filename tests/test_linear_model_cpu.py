"""``LinearModel`` and models of more than three state components without a GPU: the public class, its kernel kind and routing
flags, the packed parameter row of ``PF_HID_LINEAR_MAT``, and the torch route's arithmetic teacher-forced against the reference's
fixtures (``tools/make_golden_linear.py``)."""
import pytest
import torch
from torch.distributions import Independent, Normal

from tests import linear_cases as LC


def _inc(d, scale=1.0):
    return Independent(Normal(torch.tensor(0.0, dtype=torch.float64), torch.tensor(scale, dtype=torch.float64)).expand(torch.Size([d])), 1)


def _init(d):
    return lambda *_: Independent(Normal(torch.zeros(d, dtype=torch.float64), torch.ones(d, dtype=torch.float64)), 1)


def test_linear_model_is_public_and_computes_its_mean_scale():
    from pyfilter_amd.timeseries import LinearModel, TimeseriesState

    d = 4
    a = torch.randn(d, d, dtype=torch.float64)
    b, s = torch.randn(d, dtype=torch.float64), torch.rand(d, dtype=torch.float64) + 0.1
    x = torch.randn(7, 3, d, dtype=torch.float64)
    ts_ = TimeseriesState(0, x, torch.Size([d]))
    loc, scale = LinearModel((a, b, s), _inc(d), _init(d)).mean_scale(ts_)
    torch.testing.assert_close(loc, b + x @ a.T, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(scale, s.expand_as(loc))
    loc2, _ = LinearModel((a, s), _inc(d), _init(d)).mean_scale(ts_)  # (a, s): b = 0
    torch.testing.assert_close(loc2, x @ a.T, rtol=1e-12, atol=1e-12)
    loc3, _ = LinearModel((torch.full((d,), 0.5, dtype=torch.float64), s), _inc(d), _init(d)).mean_scale(ts_)  # elementwise
    torch.testing.assert_close(loc3, 0.5 * x)


def test_kernel_kind_and_routes():
    from pyfilter_amd import _lib as L
    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.timeseries import LinearModel, models

    d = 4
    lm = LinearModel((torch.eye(d, dtype=torch.float64), 0.1 * torch.ones(d, dtype=torch.float64)), _inc(d), _init(d))
    kind = lm.kernel_kind
    assert kind.hid_kind == L.HID_LINEAR_MAT and kind.dim == d and not kind.fused
    ssm = ts.LinearStateSpaceModel(lm, (torch.eye(2, d, dtype=torch.float64), 0.2 * torch.ones(2, dtype=torch.float64)), torch.Size([2]))
    assert ssm.kernel_kind.hid_kind == L.HID_LINEAR_MAT and ssm.kernel_kind.obs_dim == 2 and not ssm.kernel_kind.fused
    # increments other than N(0, 1), or more than 8 components: no kernel kind (torch model arithmetic)
    assert LinearModel((torch.eye(d), torch.ones(d)), _inc(d, 2.0), _init(d)).kernel_kind is None
    assert LinearModel((torch.eye(9), torch.ones(9)), _inc(9), _init(9)).kernel_kind is None
    big_o = ts.LinearStateSpaceModel(lm, (torch.ones(9, d, dtype=torch.float64), torch.ones(9, dtype=torch.float64)), torch.Size([9]))
    assert big_o.kernel_kind is None
    # the random walk: D <= 3 keeps its fused kind, 4 .. 8 the matrix kind, beyond that none
    rw3 = models.RandomWalk(torch.ones(3), dim=3)
    assert rw3.kernel_kind.hid_kind == L.HID_LINEAR and rw3.kernel_kind.fused
    rw8 = models.RandomWalk(torch.ones(8), dim=8)
    assert rw8.kernel_kind.hid_kind == L.HID_LINEAR_MAT and rw8.kernel_kind.dim == 8 and not rw8.kernel_kind.fused
    assert models.RandomWalk(torch.ones(10), dim=10).kernel_kind is None
    assert models.RandomWalk(torch.ones(5)).kernel_kind.dim == 1  # (dim is inferred for 2 or 3 components only, as before)
    # a user lambda of more than three components has no kind; the fused kinds at D, O <= 3 are unchanged
    user = ts.AffineProcess(lambda x, a, s: (x.value @ a.T, s), (torch.eye(d), torch.ones(d)), _inc(d), _init(d))
    assert ts.LinearStateSpaceModel(user, (torch.eye(2, d), torch.ones(2)), torch.Size([2])).kernel_kind is None
    lg = ts.LinearStateSpaceModel(models.RandomWalk(torch.ones(2), dim=2), (torch.eye(2), torch.ones(2)), torch.Size([2]))
    assert lg.kernel_kind.fused and lg.kernel_kind.hid_kind == L.HID_LINEAR


def test_packed_parameter_row_of_the_matrix_kind():
    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.timeseries import LinearModel
    from pyfilter_amd.timeseries.models import pack_params

    d, o, b = 5, 3, 2
    a = torch.randn(b, d, d, dtype=torch.float64)
    off, s = torch.randn(d, dtype=torch.float64), torch.rand(b, d, dtype=torch.float64)
    ao, bo, so = torch.randn(o, d, dtype=torch.float64), torch.randn(o, dtype=torch.float64), torch.rand(o, dtype=torch.float64)
    ssm = ts.LinearStateSpaceModel(LinearModel((a, off, s), _inc(d), _init(d)), (ao, bo, so), torch.Size([o]))
    rows = pack_params(ssm, b, torch.float64, torch.device("cpu"))
    assert rows.shape == (b, d * d + 2 * d + o * d + 2 * o)
    for i in range(b):
        want = torch.cat([a[i].reshape(-1), off, s[i], ao.reshape(-1), bo, so])
        assert torch.equal(rows[i], want)


def _teacher_forced(name, device):
    """From the reference's state t (resampled with its recorded uniform), the product's torch-route proposal - the model written
    as a plain AffineProcess lambda - must put the reference's recorded normals where the reference's particles are and give the
    reference's weights (NaN observation: propagate only)."""
    from pyfilter_amd.filters.particle import proposals
    from pyfilter_amd.filters.particle.proposals.linear import _ObservationUpdate
    from pyfilter_amd.timeseries import TimeseriesState

    filt_name, prop_name, ess, _ = LC.CASES[name]
    g = LC.load(name, "f64")
    ssm = LC.build_ssm(name, g, torch.float64, device, how="lambda")
    assert ssm.kernel_kind is None
    prop = {"lgo": proposals.LinearGaussianObservations, "bootstrap": proposals.Bootstrap}[prop_name]()
    prop.set_model(ssm)
    n, b = g["x0"].shape[:2]
    x, w = g["x0"].double(), torch.zeros(n, b, dtype=torch.float64)
    for t in range(g["y"].shape[0]):
        y, z = g["y"][t].double().to(device), g["z_tape"][t].double().to(device)
        idx = g["step_idx"][t]
        if filt_name == "sisr":
            # the reference's predict (sisr.py): the filters whose ESS fell below the threshold are resampled - with the ancestors
            # the fixture recorded - and restart from zero weights; the others carry particles and weights as they are
            W = torch.softmax(w, 0)
            mask = 1.0 / W.square().sum(0) < ess * n
            xr = torch.where(mask.view(1, b, 1), x.gather(0, idx.unsqueeze(-1).expand_as(x)), x)
            wr = torch.where(mask.view(1, b), torch.zeros_like(w), w)
        else:
            xr = x.gather(0, idx.unsqueeze(-1).expand_as(x))  # (the APF resamples at every move, apf.py)
        st = TimeseriesState(t, xr.to(device), ssm.hidden.event_shape)
        mean, scale = ssm.hidden.mean_scale(st)
        x_ref = g["step_x"][t].double().to(device)
        if torch.isnan(y).all():  # propagate only, weights carried (filters/base.py:212, particle/state.py:38-42)
            torch.testing.assert_close(mean + scale * z, x_ref, rtol=1e-9, atol=1e-12)
            torch.testing.assert_close(wr, g["step_w"][t].double(), rtol=1e-9, atol=1e-9)
        else:
            if prop_name == "lgo":
                kernel = _ObservationUpdate(ssm, scale).posterior(y, mean)
                torch.testing.assert_close(kernel.loc + (kernel.scale_tril @ z.unsqueeze(-1)).squeeze(-1), x_ref, rtol=1e-9, atol=1e-11)
                wi = prop._weight_with_kernel(y, ssm.hidden.build_density(st), st.copy(values=mean).propagate_from(values=x_ref), kernel)
            else:
                torch.testing.assert_close(mean + scale * z, x_ref, rtol=1e-9, atol=1e-11)
                wi = ssm.build_density(st.propagate_from(values=x_ref)).log_prob(y)
            if filt_name == "sisr":
                torch.testing.assert_close(wi.cpu() + wr, g["step_w"][t].double(), rtol=1e-9, atol=1e-9)
            else:  # APF (apf.py): the weight less the pre-weight the ancestor was drawn with, taken at the un-resampled particles
                pre = prop.pre_weight(y, TimeseriesState(t, x.to(device), ssm.hidden.event_shape)).cpu()
                torch.testing.assert_close(wi.cpu() - pre.gather(0, idx), g["step_w"][t].double(), rtol=1e-9, atol=1e-9)
        x, w = g["step_x"][t].double(), g["step_w"][t].double()


@pytest.mark.parametrize("name", list(LC.CASES))
def test_torch_route_teacher_forced_against_the_reference(name):
    _teacher_forced(name, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LC.CASES))
def test_torch_route_teacher_forced_against_the_reference_gpu(name):
    _teacher_forced(name, "cuda")
