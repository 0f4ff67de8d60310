"""The nested proposal without a GPU: the float64 oracle (``tests/nested_oracle.py``) reproduces every float64 fixture recorded
from the unmodified reference (``tools/make_golden_nested.py``), and the package's Python / C surface of the feature exists."""
import os

import pytest
import torch

from oracle.cases import build_spec
from tests import nested_oracle
from tests.nested_oracle import assert_weights_match
from tests.helpers import load_golden
from tools.make_golden_nested import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_CASES = [c for c in CASES if "f64" in c["dtypes"]]


@pytest.mark.parametrize("case", F64_CASES, ids=lambda c: c["name"])
def test_oracle_matches_reference(case):
    g = load_golden(case["name"], "f64")
    assert int(g["num_samples"]) == case["M"]
    spec = build_spec(case, torch.float64)
    out = nested_oracle.batch_filter(spec, case["filter"], case["M"], g["y"], g["x0"], g["z_tape"].double(), g["u_tape"].double(),
                                     g["v_tape"].double(), case["ess_threshold"])
    assert torch.equal(out["step_idx"], g["step_idx"].long()), "ancestors differ from the reference"
    assert torch.equal(out["step_pick"], g["step_pick"].long()), "picks differ from the reference"
    tol = dict(rtol=1e-9, atol=1e-9)
    for k in ("step_x", "step_ll", "filter_means", "loglikelihood"):
        torch.testing.assert_close(out[k], g[k], equal_nan=True, **tol)
    assert_weights_match(out["step_w"], g["step_w"], **tol)


def test_fixture_shapes_and_sizes():
    for case in CASES:
        for dt in case["dtypes"]:
            path = os.path.join(ROOT, "tests", "golden", f"{case['name']}_{dt}.npz")
            assert os.path.getsize(path) < (1 << 20)
            g = load_golden(case["name"], dt)
            t, m, n, b = case["T"], case["M"], case["N"], case["B"]
            assert tuple(g["z_tape"].shape[:4]) == (t, m, n, b) and tuple(g["v_tape"].shape) == (t, n, b)
            assert tuple(g["u_tape"].shape) == (t, b) and tuple(g["step_pick"].shape) == (t, n, b)
            for s in case.get("nan_steps", ()):
                assert bool((g["step_pick"][s] == -1).all())


def test_proposal_class():
    from pyfilter_amd.filters.particle import proposals

    p = proposals.NestedProposal(7)
    assert isinstance(p, proposals.Proposal) and p._KERNEL_PROPOSAL is None
    q = p.copy()
    assert type(q) is proposals.NestedProposal and q.num_samples == 7 and isinstance(q.num_samples, int)
    with pytest.raises(ValueError):
        proposals.NestedProposal(0)
    f = lambda mod, state: state  # noqa: E731
    assert proposals.NestedProposal(3, pre_weight_func=f).copy()._pre_weight_func is f


def test_hint_defaults_on():
    from pyfilter_amd.hints import RunHints

    assert RunHints().nested_kernel is True


def test_entry_point_declared():
    from pyfilter_amd import _lib

    assert "pf_nested_sample_and_weight" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "pf_amd.h")) as f:
        header = f.read()
    assert "int pf_nested_sample_and_weight(" in header and "#define PF_NESTED_MAX 256" in header
    assert _lib.NESTED_MAX == 256 and _lib.ABI_VERSION == 4


def test_apply_mapping_restores_the_nested_hint():
    from pyfilter_amd.hints import RunHints

    h = RunHints()
    h.nested_kernel = False
    assert h.apply_mapping({}).nested_kernel is True
    assert h.apply_mapping({"PF_NO_NESTED_KERNEL": "1"}).nested_kernel is False


@pytest.mark.parametrize("name", ["nested_lorenz_sisr", "nested_sv_sisr", "nested_rw2d_apf"])
def test_torch_route_in_slices_is_the_torch_route(name, monkeypatch):
    """The torch route walks the particles in slices of at most ``TORCH_CANDIDATES`` candidates: the same picks and - to float64
    rounding, 1e-13: torch's vectorised exp / log / sin round an element differently in the body and in the tail of a tensor - the
    same numbers as in one piece (here slices of 37 particles: ragged, a last one shorter)."""
    from pyfilter_amd.filters.particle.proposals import NestedProposal
    from tests import nested_cases as nc

    call = next(c for c in nc.teacher_forced("f64") if c.name.startswith(name))
    whole = nc.torch_route(call)
    per_particle = call.x.numel() // call.n
    monkeypatch.setattr(NestedProposal, "TORCH_CANDIDATES", 37 * call.m * per_particle // max(call.b, 1))
    sliced = nc.torch_route(call)
    assert torch.equal(whole[2], sliced[2])
    for a, b in zip(whole[:2], sliced[:2]):
        torch.testing.assert_close(a, b, rtol=1e-13, atol=1e-13)
    assert nc.weight_error(sliced[1], call.ref_w) <= 1e-12
    assert nc.weight_error(whole[1], call.ref_w) <= 1e-12 and nc.pick_mismatch(whole[2], call.ref_pick) == 0.0


def test_running_sum_that_never_passes_keeps_the_last_live_candidate():
    """``v = 1`` stands in for a rounding that leaves the last running sum <= v sum: the pick is the last candidate of positive
    weight - here the one before the last, whose normal of -50 makes a negative (invalid) stochastic-volatility candidate."""
    from tests import nested_cases as nc

    call = nc.last_candidate_invalid(torch.float64)
    assert bool((call.ref_pick == call.m - 2).all())
    _, w, pick = nc.torch_route(call)
    assert bool((pick == call.m - 2).all()) and bool(w.isfinite().all())
