"""``pf_path_score_linear`` (``k_score_linmat_part`` / ``k_score_linmat_final``, ``csrc/pf_linear_smooth.hpp``) against the float64
oracle of ``tests/linmat_score_oracle.py`` on trajectories simulated from the models themselves, and ``path_score`` /
``GradientBasedProposal`` on a ``LinearModel`` end to end.

Tolerances are ``tests/test_score_parity_gpu.py``'s.  float64: ``|kernel - oracle| <= 1e-10 A_k`` per row slot (and for the value),
``A_k = 1/N sum |term|``: kernel and oracle evaluate the same terms in double and differ by the order of the sums, amplified by the
cancellation in ``x_t - loc`` which the oracle asserts to be at most 1e3.  float32 storage: four times the error of the reference
expression evaluated in float32 (torch autograd on the CPU) against the float64 oracle at the same float32-exact inputs, per slot
the maximum over the filters, plus ``64 eps32 A_k`` - computed from the oracle, never from the kernel."""
import ctypes as C
import functools
import math

import pytest
import torch
from torch.distributions import Independent, LogNormal, Normal

from pyfilter_amd import _lib as L
from pyfilter_amd import ops
from tests import linmat_cases as LC
from tests import linmat_score_oracle as lso

pytestmark = pytest.mark.gpu

EPS32 = torch.finfo(torch.float32).eps
DTYPES = (torch.float64, torch.float32)
DIMS = ((1, 1), (2, 3), (4, 2), (5, 5), (8, 8), (8, 1), (1, 8))
# (S, N, B): the shortest call and a single path; below / above one workgroup of 256 paths; a time axis cut into chunks
SHAPES = ((2, 1, 1), (3, 255, 2), (9, 257, 3), (40, 300, 2))
CHUNKED = (40, 300, 2)


def score_plan(n, b, s):
    """``score_plan`` of ``csrc/pf_score.hpp``: ``(tiles, chunks, len)``."""
    tiles = (n + 255) // 256
    steps = s - 1
    want = (1024 + tiles * b - 1) // (tiles * b)
    chunks = max(1, min(want, steps // 8, 1024))
    length = (steps + chunks - 1) // chunks
    return tiles, (steps + length - 1) // length, length


@functools.lru_cache(maxsize=None)
def case(d, o, s, n, b, by, nan=""):
    """Inputs and oracle of one case, computed once: ``(inputs, y, oracle64, reference32)``."""
    inp = lso.Inputs(d, o, s, n, b, by=by, seed=11)
    y = inp.y.clone()
    if nan == "skip":
        y[(s - 1) // 2] = float("nan")
    elif nan == "partial":  # one element of the last filter's row (a shared row: of everybody's)
        y[(s - 1) // 2, by - 1, 0] = float("nan")
    ref = lso.score(d, o, inp.rows, inp.paths, y)
    ref32 = lso.score(d, o, inp.rows, inp.paths, y, dtype=torch.float32, per_term=False)
    return inp, y, ref, ref32


def bounds(ref, ref32, dtype):
    """``(bound of the value (B,), bound of the gradient (B, NP))``."""
    if dtype == torch.float64:
        return 1e-10 * ref["A_value"], 1e-10 * ref["A_grad"]
    ev = torch.nan_to_num((ref32["value"].double() - ref["value"]).abs(), nan=0.0).max(0)[0]
    eg = torch.nan_to_num((ref32["grad"].double() - ref["grad"]).abs(), nan=0.0).max(0)[0]
    return 4.0 * ev + 64.0 * EPS32 * ref["A_value"], 4.0 * eg + 64.0 * EPS32 * ref["A_grad"]


def run_kernel(d, o, inp, y, dtype):
    rows, paths, _ = inp.soa(dtype, "cuda")
    value, grad = ops.path_score_linear(LC.kernel_kind(d, o), rows, paths, y.to(device="cuda", dtype=dtype))
    assert value.dtype == torch.float64 and grad.dtype == torch.float64 and grad.shape == (inp.b, lso.n_params(d, o))
    return value.cpu(), grad.cpu()


def check(d, o, s, n, b, by, dtype, nan=""):
    inp, y, ref, ref32 = case(d, o, s, n, b, by, nan)
    value, grad = run_kernel(d, o, inp, y, dtype)
    bv, bg = bounds(ref, ref32, dtype)
    ev, eg = (value - ref["value"]).abs(), (grad - ref["grad"]).abs()
    print(f"linmat-score-parity: D{d}-O{o} S={s} N={n} B={b} By={by} {str(dtype)[6:]} {nan}: value err/bound {float((ev / bv).max()):.3g}, "
          f"grad err/bound {float((eg / bg.clamp_min(1e-300)).max()):.3g}")
    assert bool((ref["A_grad"] > 0).all())  # (every slot of this kind's row is read)
    assert bool((ev <= bv).all()), (ev, bv)
    assert bool((eg <= bg).all()), (eg / bg.clamp_min(1e-300)).max()
    return value, grad


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("s,n,b", SHAPES, ids=[f"{s}x{n}x{b}" for s, n, b in SHAPES])
@pytest.mark.parametrize("d,o", DIMS, ids=[f"D{d}-O{o}" for d, o in DIMS])
def test_value_and_every_gradient_slot(d, o, s, n, b, dtype):
    if (s, n, b) == CHUNKED:
        tiles, chunks, length = score_plan(n, b, s)
        assert (tiles, chunks, length) == (2, 4, 10)  # four time chunks, the last ragged (9 transitions)
        # ... and the library's own plan: its slab is four times the slab of the same call with 8 transitions (one chunk)
        cut, whole = C.c_size_t(0), C.c_size_t(0)
        assert L.load().pf_path_score_linear_workspace_bytes(n, b, s, d, o, C.byref(cut)) == 0
        assert L.load().pf_path_score_linear_workspace_bytes(n, b, 9, d, o, C.byref(whole)) == 0
        assert cut.value == 4 * whole.value > 0
    for by in sorted({1, b}):
        check(d, o, s, n, b, by, dtype)


@pytest.mark.parametrize("d,o", ((4, 2), (8, 8)), ids=("D4-O2", "D8-O8"))
def test_nan_rows(d, o):
    """An all-NaN row is skipped and matches the oracle; a half-NaN row in one filter's series (``y_rows = B``) gives NaN value and
    gradient for that filter only, with ``y_rows = 1`` for all filters."""
    s, n, b = CHUNKED
    for dtype in DTYPES:
        for by in (1, b):
            value, _ = check(d, o, s, n, b, by, dtype, nan="skip")
            assert torch.isfinite(value).all()
            inp, y, ref, ref32 = case(d, o, s, n, b, by, "partial")
            value, grad = run_kernel(d, o, inp, y, dtype)
            hit = torch.tensor([True] * b if by == 1 else [False] * (b - 1) + [True])
            assert value.isnan().tolist() == hit.tolist() and ref["value"].isnan().tolist() == hit.tolist()
            assert grad[hit].isnan().all() and ref["grad"][hit].isnan().all()
            bv, bg = bounds(ref, ref32, dtype)
            assert bool(((value - ref["value"]).abs()[~hit] <= bv[~hit]).all())
            assert bool(((grad - ref["grad"]).abs()[~hit] <= bg[~hit]).all())


def test_result_is_a_function_of_inputs_and_shape():
    d, o = 8, 8
    inp, y, _, _ = case(d, o, *CHUNKED, 1)
    first = run_kernel(d, o, inp, y, torch.float32)
    again = run_kernel(d, o, inp, y, torch.float32)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


# ---------------------------------------------------------------------------------------------------------------- by name
def _cv_data(t_obs=12):
    """A constant-velocity track observed in its two positions: phi = 0.9, q = 0.3, r = 0.5 (CPU generator)."""
    gen = torch.Generator().manual_seed(2024)
    x, ys = torch.tensor([0.0, 0.0, 1.0, -0.5], dtype=torch.float64), []
    for _ in range(t_obs):
        x = torch.stack((x[0] + x[2], x[1] + x[3], 0.9 * x[2], 0.9 * x[3])) + 0.3 * torch.tensor([0.5, 0.5, 1.0, 1.0]) * torch.randn(
            4, generator=gen, dtype=torch.float64)
        ys.append(x[:2] + 0.5 * torch.randn(2, generator=gen, dtype=torch.float64))
    return torch.stack(ys)


def _cv_builder(dtype, device="cuda"):
    """``LinearModel`` whose A, s and observation scale depend on named parameters: velocities decay by ``phi``, process noise ``q``
    (half of it on the positions), observation noise ``r`` - one value per filter each."""
    t = lambda v: torch.tensor(v, device=device, dtype=dtype)  # noqa: E731
    shift = t([[1.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    decay = t([[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    noise, h = t([0.5, 0.5, 1.0, 1.0]), t([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]])
    m0, s0 = t([0.0, 0.0, 1.0, -0.5]), t([0.5, 0.5, 0.5, 0.5])

    def build(theta):
        from pyfilter_amd import timeseries as ts
        from pyfilter_amd.timeseries import models

        phi, q, r = (theta[k].reshape(-1) for k in ("phi", "q", "r"))
        a = shift + phi.reshape(-1, 1, 1) * decay              # (B, 4, 4)
        s = q.reshape(-1, 1) * noise                           # (B, 4)
        inc = Independent(Normal(t(0.0), t(1.0)).expand(torch.Size([4])), 1)
        hidden = models.LinearModel((a, torch.zeros_like(s), s), inc, lambda *_: Independent(Normal(m0, s0), 1))
        return ts.LinearStateSpaceModel(hidden, (h, t([0.0, 0.0]), r.reshape(-1, 1) * t([1.0, 1.0])), torch.Size([2]))

    return build


def _cv_priors():
    return {"phi": LogNormal(math.log(0.9), 0.05), "q": LogNormal(math.log(0.3), 0.2), "r": LogNormal(math.log(0.5), 0.2)}


def _cv_filtered(dtype, chains=4, particles=256, seed=9):
    from types import SimpleNamespace

    from pyfilter_amd.filters.particle import SISR
    from pyfilter_amd.inference import ThetaParticles

    y = _cv_data().to(device="cuda", dtype=dtype)
    theta = ThetaParticles(_cv_priors(), chains, "cuda", dtype)
    theta.initialize_parameters(torch.Generator().manual_seed(3))
    filt = SISR(_cv_builder(dtype), particles, record_states=True, seed=seed)
    filt.set_batch_shape(torch.Size([chains]))
    filt.initialize_model(theta)
    return y, theta, filt, SimpleNamespace(filter_state=filt.batch_filter(y, bar=False))


def test_gradient_by_name():
    """``path_score(theta=..., route="kernel")`` on the constant-velocity ``LinearModel`` against ``route="torch"`` in float64 - to
    the bound of the kernel-against-torch comparisons of ``tests/test_gradient_proposal_gpu.py``, the parity test's float64 bound
    carried to the names plus 1e-12 of the same magnitudes for the torch route's own rounding: ``phi`` is the slots A[2][2] and
    A[3][3], ``q`` the four transition scales through (0.5, 0.5, 1, 1), ``r`` the two observation scales.  ``route="auto"`` on the
    GPU is ``"kernel"`` bit for bit."""
    from pyfilter_amd.timeseries.models import pack_params

    y, theta, filt, state = _cv_filtered(torch.float64)
    assert filt.ssm.kernel_kind.hid_kind == L.HID_LINEAR_MAT
    paths = filt.smooth(state.filter_state.states, "fl")
    named = {n: theta[n] for n in theta.names()}
    value, grads = filt.path_score(paths, y, theta=named, route="kernel")
    want_value, want = filt.path_score(paths, y, theta=named, route="torch")
    auto_value, auto = filt.path_score(paths, y, theta=named)
    assert value.dtype == torch.float64 and torch.equal(auto_value, value) and all(torch.equal(auto[n], grads[n]) for n in named)
    assert torch.equal(filt.path_score(paths, y), value)
    b, d, o = 4, 4, 2
    rows = pack_params(filt.ssm, b, torch.float64, "cuda").cpu()
    ref = lso.score(d, o, rows, paths.cpu(), y.cpu().reshape(-1, 1, o))
    A = ref["A_grad"]
    s_at, so_at = d * d + d, d * d + 2 * d + o * d + o
    noise = torch.tensor([0.5, 0.5, 1.0, 1.0], dtype=torch.float64)
    scale = {"phi": A[:, 2 * d + 2] + A[:, 3 * d + 3], "q": (A[:, s_at:s_at + d] * noise).sum(-1), "r": A[:, so_at:so_at + o].sum(-1)}
    assert bool(((value - want_value).abs().cpu() <= (1e-10 + 1e-12) * (ref["A_value"] + want_value.abs().cpu())).all())
    for k in named:
        err, bound = (grads[k] - want[k]).abs().cpu().reshape(-1), (1e-10 + 1e-12) * scale[k]
        print(f"linmat-score-parity: by name {k}: err / bound {float((err / bound).max()):.3g}")
        assert grads[k].shape == named[k].shape and bool((err <= bound).all()), (k, err, bound)
        assert bool((want[k].abs().cpu().reshape(-1) > 100.0 * bound).all())  # (the comparison sees the gradient)


def test_gradient_proposal_on_kernels_end_to_end():
    """``PMMH`` with ``GradientBasedProposal(route="kernel")`` on the matrix model, 4 chains x 256 particles x T = 12: the run
    completes with an acceptance rate inside (0, 1), and one move's launch trace holds ``pf_smooth_ffbs_linear`` and
    ``pf_path_score_linear``."""
    from pyfilter_amd.filters.particle import SISR
    from pyfilter_amd.inference import PMMH, GradientBasedProposal

    dtype = torch.float32
    y = _cv_data().to(device="cuda", dtype=dtype)
    filt = SISR(_cv_builder(dtype), 256, record_states=True, seed=21)
    alg = PMMH(filt, 20, _cv_priors(), num_chains=4, proposal=GradientBasedProposal(scale=0.05, route="kernel"), seed=1)
    res = alg.fit(y)
    assert res.samples.shape == (21, 4, 3) and torch.isfinite(res.samples).all()
    rate = float(res.acceptance_rate().double().mean())  # (accepted moves per chain over the 20 moves)
    print(f"linmat-score-parity: PMMH on kernels, acceptance rate {rate:.3f}")
    assert 0.0 < rate < 1.0

    y, theta, filt, state = _cv_filtered(dtype)
    GradientBasedProposal(scale=0.05, route="kernel").build(theta, state, filt, y)
    after = ops.debug_launch_trace(8)
    names = [r["ENTRY"] for r in after[-2:]]
    assert names == ["pf_smooth_ffbs_linear", "pf_path_score_linear"], after
    assert after[-2]["SPEC"] == 20 and after[-1]["SPEC"] == 21 and after[-1]["D"] == 4 and after[-1]["tbytes"] == 4
    GradientBasedProposal(scale=0.05).build(theta, state, filt, y)  # ("auto": the torch logits, then the score kernel)
    assert [r["ENTRY"] for r in ops.debug_launch_trace(2)] == ["pf_path_score_linear", "pf_path_score_linear"]
    with pytest.raises(ValueError):
        GradientBasedProposal(route="hip")
