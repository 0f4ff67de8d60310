"""``pf_path_score`` (``csrc/pf_score.hpp``) against the float64 oracle of ``tests/score_oracle.py`` on trajectories simulated from
the models themselves (a CPU generator; no filter runs): every hidden kind under both observation kinds and every D / O
combination in both dtypes, particle counts around the wave and workgroup sizes, one and several filters, trajectories of 2, 3
and 17 states and one whose time axis is cut into chunks with a ragged last one, shared and per-filter observations, all-NaN
and half-NaN observation rows, and the refused kinds.

Tolerances.  float64: ``|kernel - oracle| <= 1e-10 A_k`` per row slot (and for the value), ``A_k = 1/N sum |term|``.  Kernel and
oracle evaluate the same terms in double; they differ by the order of the sum and a few ulp in sin / cos / exp, amplified by the
cancellation in ``x_t - loc``, which the oracle asserts to be at most 1e3: about 1e-12, two orders inside the bound.
float32: not derivable - the reference's own float32 error is measured instead: torch float32 autograd of the same expression on
the CPU against the float64 oracle at the same (float32-exact) inputs, per slot the maximum over the filters; the kernel, whose
arithmetic is double, gets four times that figure plus a floor of ``64 eps32 A_k`` where the reference's error happens to be
tiny.  The bound is computed from the reference at run time, never from the kernel.  Measured figures per kind:
``profiles/path_score_parity.txt`` (``tools/path_score_parity.py``)."""
import functools

import pytest
import torch

from pyfilter_amd import _lib as L
from pyfilter_amd import ops
from tests import score_oracle as so

pytestmark = pytest.mark.gpu

EPS32 = torch.finfo(torch.float32).eps
DTYPES = (torch.float64, torch.float32)
KINDS = [so.Kind(name, d, o, sv) for name in ("linear", "sine", "verhulst", "ou") for d, o, sv in
         ((1, 1, False), (1, 1, True), (2, 1, False), (2, 2, False), (3, 1, False), (3, 3, False))]
KINDS += [so.Kind("lorenz", 3, 1), so.Kind("lorenz", 3, 3)]
BY_NAME = {repr(k): k for k in KINDS}
EDGE_KINDS = ("sine-D1-O1-lin", "lorenz-D3-O3-lin")
# S = 20 at one workgroup per filter: 19 transitions in chunks of 10 and 9 (score_plan: floor(19 / 8) = 2 chunks, evened out) - a
# boundary and a ragged last chunk; S = 17 is two whole chunks of 8
CHUNKED_S = 20


@functools.lru_cache(maxsize=None)
def case(name, s, n, b, by, nan=""):
    """Inputs and oracle of one case, computed once: ``(inputs, y, oracle64, reference32)``."""
    kind = BY_NAME[name]
    inp = so.Inputs(kind, s, n, b, by=by, seed=11)
    y = inp.y.clone()
    if nan in ("first", "middle", "last"):
        y[{"first": 0, "middle": (s - 1) // 2, "last": s - 2}[nan]] = float("nan")
    elif nan == "partial":  # one element of the last filter's row (a shared row: of everybody's)
        y[(s - 1) // 2, by - 1, 0] = float("nan")
    ref = so.score(kind, inp.rows, inp.paths, y)
    ref32 = so.score(kind, inp.rows, inp.paths, y, dtype=torch.float32, per_term=False)
    return inp, y, ref, ref32


def bounds(ref, ref32, dtype):
    """``(bound of the value (B,), bound of the gradient (B, NP))``."""
    if dtype == torch.float64:
        return 1e-10 * ref["A_value"], 1e-10 * ref["A_grad"]
    # (the maximum over the filters that have a value: a half-observed filter is NaN on both sides)
    ev = torch.nan_to_num((ref32["value"].double() - ref["value"]).abs(), nan=0.0).max(0)[0]
    eg = torch.nan_to_num((ref32["grad"].double() - ref["grad"]).abs(), nan=0.0).max(0)[0]
    return 4.0 * ev + 64.0 * EPS32 * ref["A_value"], 4.0 * eg + 64.0 * EPS32 * ref["A_grad"]


def run_kernel(kind, inp, y, dtype):
    rows, paths, _ = inp.soa(dtype, "cuda")
    value, grad = ops.path_score(kind, rows, paths, y.to(device="cuda", dtype=dtype))
    assert value.dtype == torch.float64 and grad.dtype == torch.float64
    return value.cpu(), grad.cpu()


def check(name, s, n, b, by, dtype, nan=""):
    kind = BY_NAME[name]
    inp, y, ref, ref32 = case(name, s, n, b, by, nan)
    value, grad = run_kernel(kind, inp, y, dtype)
    bv, bg = bounds(ref, ref32, dtype)
    ev, eg = (value - ref["value"]).abs(), (grad - ref["grad"]).abs()
    print(f"{name} S={s} N={n} B={b} By={by} {str(dtype)[6:]} {nan}: value err/bound {float((ev / bv).max()):.3g}, "
          f"grad err/bound {float((eg / bg.clamp_min(1e-300)).max()):.3g}, slots with A = 0: {int((ref['A_grad'] == 0).sum())}")
    assert bool((ev <= bv).all()), (ev, bv)
    assert bool((eg <= bg).all()), (eg / bg.clamp_min(1e-300)).max()
    return value, grad


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_every_kind(name, dtype):
    check(name, 17, 65, 3, 1, dtype)


@pytest.mark.parametrize("b", (1, 3))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 1023, 1024, 1025, 2052))
@pytest.mark.parametrize("name", EDGE_KINDS)
def test_particle_counts(name, n, b):
    check(name, 3, n, b, 1, torch.float64)
    check(name, 3, n, b, 1, torch.float32)


@pytest.mark.parametrize("by", (1, 3))
@pytest.mark.parametrize("s", (2, 3, 17, CHUNKED_S))
@pytest.mark.parametrize("name", EDGE_KINDS)
def test_lengths_and_observation_rows(name, s, by):
    check(name, s, 65, 3, by, torch.float64)
    check(name, s, 65, 3, by, torch.float32)


@pytest.mark.parametrize("where", ("first", "middle", "last"))
@pytest.mark.parametrize("name", EDGE_KINDS + ("ou-D1-O1-sv",))
def test_unobserved_rows_are_skipped(name, where):
    for dtype in DTYPES:
        value, _ = check(name, CHUNKED_S, 65, 3, 3, dtype, nan=where)
        assert torch.isfinite(value).all()


@pytest.mark.parametrize("by", (1, 3))
@pytest.mark.parametrize("name", ("lorenz-D3-O3-lin", "linear-D2-O2-lin"))
def test_half_observed_row_is_nan_for_its_filters_only(name, by):
    kind = BY_NAME[name]
    for dtype in DTYPES:
        inp, y, ref, ref32 = case(name, CHUNKED_S, 65, 3, by, "partial")
        value, grad = run_kernel(kind, inp, y, dtype)
        hit = torch.tensor([True] * 3 if by == 1 else [False, False, True])
        assert value.isnan().tolist() == hit.tolist() and ref["value"].isnan().tolist() == hit.tolist()
        assert grad[hit].isnan().all() and ref["grad"][hit].isnan().all()
        bv, bg = bounds(ref, ref32, dtype)
        assert bool(((value - ref["value"]).abs()[~hit] <= bv[~hit]).all())
        assert bool(((grad - ref["grad"]).abs()[~hit] <= bg[~hit]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", EDGE_KINDS)
def test_several_tiles_and_several_chunks(name, dtype):
    """Five workgroups per filter and two time chunks, the last ragged: every index of the slab ``(chunk, tile)``."""
    check(name, CHUNKED_S, 1025, 3, 1, dtype)


def test_result_is_a_function_of_inputs_and_shape():
    kind = BY_NAME["lorenz-D3-O3-lin"]
    inp, y, _, _ = case("lorenz-D3-O3-lin", CHUNKED_S, 1025, 3, 1)
    first = run_kernel(kind, inp, y, torch.float32)
    again = run_kernel(kind, inp, y, torch.float32)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def test_refused_kinds_return_their_error_code():
    kind = so.Kind("linear", 2, 2)
    inp = so.Inputs(kind, 3, 8, 2, seed=1)
    rows, paths, y = inp.soa(torch.float64, "cuda")

    def refused(code, **changes):
        k = so.Kind("linear", 2, 2)
        for name, v in changes.items():
            setattr(k, name, v)
        with pytest.raises(L.PfAmdError, match=rf"\(code {code}\)"):
            ops.path_score(k, rows, paths, y)

    refused(-3, hid_kind=L.HID_LINEAR_MAT)
    refused(-3, hid_kind=L.HID_USER_AFFINE)
    with pytest.raises(L.PfAmdError, match="do not match the model kind"):  # (a kind of another shape never reaches a launch)
        k = so.Kind("linear", 2, 2)
        k.dim = 3
        ops.path_score(k, rows, paths, y)
    with pytest.raises(L.PfAmdError, match=r"\(code -1\)"):
        ops.path_score(kind, rows, paths[:1], y[:0])  # S < 2
    ops.path_score(kind, rows, paths, y)  # (and the call itself is fine)
