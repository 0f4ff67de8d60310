"""``k_linmat_sample_and_weight`` / ``k_linmat_pre_weight`` (``csrc/pf_linear.hpp``, kind ``PF_HID_LINEAR_MAT``) against the exact host
oracle of ``tests/linmat_oracle.py``, through ``ops.sample_and_weight_soa`` / ``ops.pre_weight_soa`` with a tape of normals: every
``D x O`` in 1..8 x 1..8 at all five entry points (optimal and bootstrap move, both first-stage weights, propagate-only) in both
dtypes; particle counts around the wave, the workgroup and several workgroups per filter with one and three filters and shared and
per-filter observation rows; the second trip of the grid stride; states at 10 and 1e3; a ladder of ``s_o / s`` down to 1e-3 (float64);
the kernels' own draws at D = 4, 5, 7, 8; bit-level determinism; and the refusals.  The cases: ``tests/linmat_cases.py``; what they
have to satisfy for the bounds to mean something: ``tests/test_linmat_oracle_cpu.py``.

Bounds.  float64 (``linmat_oracle.bounds_f64``, eps = 2^-52), per particle and component:

    tol_x = 16 eps cond_2(P) (|K||m| + |c| + |L||z|) + 4 eps |x'|        bootstrap / propagate-only: 4 eps (|m| + |s z|)
    tol_w = sum_d |d log w / d x'_d| tol_x_d + 16 eps A_w + 4 D eps cond_2(P)
    pre-weight: 16 eps A_w + 4 D eps cond_2(S)

with the magnitudes as the oracle's docstring defines them (``A_w`` counts a residual by the size of its own terms; ``|m|`` of the
bootstrap move is ``|b| + |A||x|``).  At ``s_o / s = 2`` ``cond(P)`` is 10 to 100: about 1e-13 of the particle.
float32: not derivable (constants formed in double and rounded, per-particle work in float) - measured from the reference instead:
``oracle/cpu_ref.py`` in torch float32 on the CPU at the same float32-exact inputs against the exact oracle, the maximum over the
particles of the case; the kernel gets 4 x that figure (the margin of ``tests/test_score_parity_gpu.py``) plus a floor of ``64 eps32``
x the same magnitudes.  Never from the kernel.  Every test prints ``err / bound``; the measured figures, and which tests three
single-line mutations of the kernels fail: ``profiles/linear_parity.txt`` (``tools/linmat_parity.py``).  Measured on an MI355X: the
largest float64 ``err / bound`` is 0.46 (the bootstrap move's ``4 eps``; 0.30 on the optimal proposal, at ``cond_2(P)`` = 1.4e3); the
float32 kernel's error is 0.2 .. 3.2 of the reference's at N >= 63 and up to 21 at N = 1, where a single particle's reference error is
by chance near zero and the floor is the bound - at most 0.06 of the bound anywhere.  The file runs in 11 s, the second-trip cases in
2.8 s (8 x 8 float32 move), 0.8 s, 0.6 s and 0.1 s, the oracle and the float32 reference included."""
import ctypes as C

import pytest
import torch

from pyfilter_amd import _lib as L
from pyfilter_amd import ops
from tests import linmat_cases as LC
from tests import philox_cases as PC
from tests import philox_ref as P

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DTYPES = (F64, F32)
EINVAL, EUNSUPPORTED = -1, -3  # include/pf_amd.h: PF_EINVAL, PF_EUNSUPPORTED


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A device error is sticky: nothing of this module runs on the device after one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, the remaining cases are not run: {e}", returncode=3)


def _name(dtype):
    return "f32" if dtype == F32 else "f64"


def check(c, dtype, entries=LC.ENTRY_POINTS):
    worst = {}
    for entry in entries:
        m = LC.measure(c, entry, dtype)
        ref = "".join(f" {k}_err {m[k + '_err']:.3g} (reference {m[k + '_ref']:.3g})" for k in ("x", "w") if k + "_ref" in m)
        print(f"linmat-parity: {c} {_name(dtype)} {entry}: err/bound" + "".join(f" {k} {m[k]:.3g}" for k in ("x", "w") if k in m) + ref)
        worst[entry] = m
    bad = {e: {k: m[k] for k in ("x", "w") if k in m and not m[k] <= 1.0} for e, m in worst.items()}
    assert not any(bad.values()), (repr(c), _name(dtype), {e: v for e, v in bad.items() if v})


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("d,o", LC.ALL_SHAPES)
def test_every_shape(d, o, dtype):
    check(LC.case(d, o, 65, 3, 3), dtype)


@pytest.mark.parametrize("b,y_rows", LC.EDGE_B_ROWS)
@pytest.mark.parametrize("n", LC.EDGE_N)
@pytest.mark.parametrize("d,o", LC.EDGE_SHAPES)
def test_particle_counts_filters_and_observation_rows(d, o, n, b, y_rows):
    for dtype in DTYPES:
        check(LC.case(d, o, n, b, y_rows), dtype)


@pytest.mark.parametrize("entry", ("lgo", "pre_lgo"))
@pytest.mark.parametrize("shape,dtype", LC.SECOND_TRIP, ids=lambda v: _name(v) if isinstance(v, torch.dtype) else f"{v[0]}x{v[1]}")
def test_second_trip_of_the_grid_stride(shape, dtype, entry):
    """N = 2048 x 256 + 77: the grid is capped at 2048 workgroups, so the first 77 threads make a second, ragged trip."""
    check(LC.second_trip_case(*shape), dtype, (entry,))


@pytest.mark.parametrize("level", LC.LEVELS)
@pytest.mark.parametrize("d,o", LC.LEVEL_SHAPES)
def test_states_far_from_zero(d, o, level):
    for dtype in DTYPES:
        check(LC.case(d, o, 65, 3, 3, level=level), dtype)


@pytest.mark.parametrize("ratio", LC.LADDER)
@pytest.mark.parametrize("d,o", LC.LADDER_SHAPES)
def test_conditioning_ladder_float64(d, o, ratio):
    """``s_o / s`` down to 1e-3: ``cond_2(P)`` up to ~2e7, under the cap of 1e8 (asserted on the CPU).  float64 only: the reference's
    own float32 run does not complete below 0.1."""
    check(LC.case(d, o, 65, 3, 3, ratio=ratio), F64)


# ------------------------------------------------------------------------------------------------------- bits and draws
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("d", (4, 5, 7, 8))
def test_own_draws(d, dtype):
    """``z = NULL``: ``NormalDraw<T, D>`` at D > 4 - particle ``e = b N + i`` takes the normals of flat indices ``e D .. e D + D - 1`` of
    stream NORMAL.  The call equals the taped call fed the host Philox oracle's normals, to the bars of
    ``test_philox_draws_gpu.py::test_sample_and_weight_own_draws`` (float64 1e-12 relative; float32 1e-3 on the normals: every
    ``|L|`` and ``s`` here is under 1, so 1e-3 on the particles)."""
    seed, step, n, b = PC.SEED_LOW, 6, 1003, 2
    c = LC.case(d, 3, n, b, b)
    for entry in ("lgo", "bootstrap"):
        own_x, own_w = LC.run_kernel(c, entry, dtype, own_draws=(seed, step))
        z = PC.oracle_normals(seed, P.STREAMS["NORMAL"], step, n, b, d, "float32" if dtype == F32 else "float64").to(dtype)  # (N, B, D)
        taped = LC.Case(d, 3, n, b, b)
        taped.z = z.double().numpy()
        tap_x, tap_w = LC.run_kernel(taped, entry, dtype)
        ref = tap_x.double().cpu()
        err = (own_x.double().cpu() - ref).abs()
        bar = PC.VALUE_F64 * (1.0 + ref.abs()) if dtype == F64 else torch.full_like(ref, PC.NORMAL_F32)
        print(f"linmat-parity: own draws D={d} {_name(dtype)} {entry}: largest |own - taped| x {float(err.max()):.3e}")
        assert bool((err <= bar).all()), float(err.max())
        if dtype == F64:
            own_w, tap_w = own_w.cpu(), tap_w.cpu()
            werr = float(((own_w - tap_w).abs() / (1.0 + tap_w.abs())).max())
            print(f"linmat-parity: own draws D={d} f64 {entry}: largest |own - taped| w / (1 + |w|) {werr:.3e}")
            assert werr <= PC.VALUE_F64
        other, _ = LC.run_kernel(c, entry, dtype, own_draws=(seed, step + 1))
        assert not torch.equal(other, own_x)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("d,o", LC.EDGE_SHAPES)
def test_a_call_is_a_function_of_its_inputs(d, o, dtype):
    """The same call twice gives equal bits, at every entry point; and ``weigh = 0`` gives the bootstrap move's particles bit for bit."""
    c = LC.case(d, o, 1025, 3, 3)
    first = {e: LC.run_kernel(c, e, dtype) for e in LC.ENTRY_POINTS}
    for e in LC.ENTRY_POINTS:
        again = LC.run_kernel(c, e, dtype)
        for p, q in zip(first[e], again):
            assert (p is None and q is None) or torch.equal(p, q), e
    assert torch.equal(first["propagate"][0], first["bootstrap"][0])


# ------------------------------------------------------------------------------------------------------------- refusals
def _model(hid, d, o, obs_kind, params):
    m = L.PfModel()
    m.hid_kind, m.obs_kind, m.dim, m.obs_dim, m.dt, m.inc_scale, m.params = hid, obs_kind, d, o, 1.0, 1.0, params.data_ptr()
    return m


def test_refusals_return_their_codes_and_leave_the_library_usable():
    """D or O of 9 and ``PF_OBS_SV``: ``PF_EUNSUPPORTED`` (``check_model``); a ``y_rows`` that is neither 1 nor B: ``PF_EINVAL``; the
    nested, FFBS and path-score entry points: ``PF_EUNSUPPORTED``, the forecast: ``PF_EINVAL`` (``include/pf_amd.h``) - all before
    any launch, the outputs untouched; and a good call made afterwards still works."""
    lib = L.load()
    n, b, dm = 64, 2, 9
    dev = "cuda"
    params = torch.ones(512, dtype=F64, device=dev)
    x = torch.zeros((dm, b, n), dtype=F64, device=dev)
    y = torch.zeros((b, dm), dtype=F64, device=dev)
    x_out, w_out = torch.full((dm, b, n), -77.0, dtype=F64, device=dev), torch.full((b, n), -77.0, dtype=F64, device=dev)

    def saw(d, o, obs_kind=L.OBS_LINEAR, y_rows=1, proposal=L.PROP_LGO):
        m = _model(L.HID_LINEAR_MAT, d, o, obs_kind, params)
        return lib.pf_sample_and_weight(C.byref(m), proposal, 1, x.data_ptr(), y.data_ptr(), y_rows, x.data_ptr(), 0, 0, x_out.data_ptr(),
                                        w_out.data_ptr(), n, b, L.PF_F64, L.stream_ptr())

    def pre(d, o, obs_kind=L.OBS_LINEAR, y_rows=1, proposal=L.PROP_LGO):
        m = _model(L.HID_LINEAR_MAT, d, o, obs_kind, params)
        return lib.pf_pre_weight(C.byref(m), proposal, x.data_ptr(), y.data_ptr(), y_rows, w_out.data_ptr(), n, b, L.PF_F64, L.stream_ptr())

    for call in (saw, pre):
        assert call(9, 2) == EUNSUPPORTED and call(2, 9) == EUNSUPPORTED and call(0, 2) == EUNSUPPORTED and call(2, 0) == EUNSUPPORTED
        for prop in (L.PROP_LGO, L.PROP_BOOTSTRAP):
            assert call(1, 1, obs_kind=L.OBS_SV, proposal=prop) == EUNSUPPORTED
        assert call(4, 2, y_rows=3) == EINVAL and call(4, 2, y_rows=0) == EINVAL  # (B = 2)
    # the entry points that do not serve this kind
    m = _model(L.HID_LINEAR_MAT, 2, 2, L.OBS_LINEAR, params)
    pick = torch.zeros((b, n), dtype=torch.int32, device=dev)
    assert lib.pf_nested_sample_and_weight(C.byref(m), 4, x.data_ptr(), y.data_ptr(), 1, None, None, 1, 0, x_out.data_ptr(), w_out.data_ptr(),
                                           pick.data_ptr(), n, b, L.PF_F64, L.stream_ptr()) == EUNSUPPORTED
    hist, logw = torch.zeros((3, 2, b, n), dtype=F64, device=dev), torch.zeros((3, b, n), dtype=F64, device=dev)
    out = torch.full((3, 2, b, n), -77.0, dtype=F64, device=dev)
    assert lib.pf_smooth_ffbs(C.byref(m), hist.data_ptr(), logw.data_ptr(), x.data_ptr(), None, 1, out.data_ptr(), 3, n, b, L.PF_F64,
                              L.stream_ptr()) == EUNSUPPORTED
    kind = LC.kernel_kind(2, 2)
    rows = torch.ones((b, 16), dtype=F64, device=dev)  # (NP of this kind at D = O = 2 is the built-in kinds' 4 D + O D + 2 O)
    with pytest.raises(L.PfAmdError, match=r"pf_forecast failed: invalid argument \(code -1\)"):
        ops.forecast_soa(kind, rows, 3, torch.zeros((2, b, n), dtype=F64, device=dev), None)
    with pytest.raises(L.PfAmdError, match=r"\(code -3\)"):
        ops.path_score(kind, rows, hist, torch.zeros((2, 2), dtype=F64, device=dev))
    torch.cuda.synchronize()
    assert bool((x_out == -77.0).all() and (w_out == -77.0).all() and (out == -77.0).all())
    # ... and the library still serves a good call
    check(LC.case(4, 2, 65, 3, 3), F64, ("lgo", "pre_lgo"))
