"""NESS pinned against the reference, CPU leg: the PRODUCT's ``pyfilter_amd.inference.ness`` on its torch route (``NESS.step``,
``FixedWidthNESS``, ``OnlineKernel.update``, ``robust_var`` and the four jittering kernels) replays the event logs recorded from
the unmodified reference (``tools/make_golden_ness.py``) - same draws at the same points, every intermediate quantity compared.
The particle filter underneath is the oracle-backed stand-in of ``tests/test_inference_reference_cpu.py``;
``tests/test_ness_gpu.py`` runs the same replays on the HIP filters and kernels.  Below them: the host logic."""
import types

import pytest
import torch

from tests.ness_replay import NESS_CASES, priors, replay_ness
from tests.test_inference_reference_cpu import _oracle_filter


@pytest.mark.parametrize("name", sorted(NESS_CASES))
def test_ness_replays_the_reference_event_log(name):
    updates, routes = replay_ness(name, _oracle_filter, "cpu")
    assert updates >= 3 and routes == {"torch"}


def _bare(cls, **attrs):
    """An algorithm object without filters: what ``_step`` touches, the kernel and the move replaced by recorders."""
    from pyfilter_amd.inference import ness

    calls = []
    alg = cls.__new__(cls)
    alg.theta = alg.filter = alg._gen = None
    alg._kernel = types.SimpleNamespace(update=lambda theta, filt, state, generator=None: (calls.append("update"), state)[1])
    for k, v in attrs.items():
        setattr(alg, k, v)
    state = types.SimpleNamespace(stats=torch.tensor([10.0, 1.0]), current_iteration=0)
    return ness, alg, state, calls


def test_the_update_test_reads_the_ess_the_previous_observation_left(monkeypatch):
    """``ness.py:50-58``: test, update, move, ``w += ll`` - SMC^2 tests AFTER the move.  B = 10, threshold 0.9."""
    from pyfilter_amd.inference import NESS

    ness, alg, state, calls = _bare(NESS, _threshold=0.9 * 10)
    pairs = iter([(9.5, 1.0), (5.0, 1.0), (9.9, 1.0), (9.9, 0.0), (9.9, 1.0), (8.99, 1.0)])
    monkeypatch.setattr(ness, "online_move", lambda a, y, s: (calls.append("move"), next(pairs))[1])
    for t in range(6):
        state = alg.step(None, state)
    # initial ESS 10: no update; 9.5: none; 5.0 -> update before move 2; 9.9: none; a non-finite weight -> update before move 4
    assert calls == ["move", "move", "update", "move", "move", "update", "move", "move"]
    assert state.current_iteration == 6
    assert alg.do_update_particles(state)  # (8.99 < 9: the next step starts with an update)


def test_fixed_width_ness_counts_calls_and_watches_the_weights(monkeypatch):
    from pyfilter_amd.inference import FixedWidthNESS

    ness, alg, state, calls = _bare(FixedWidthNESS, _bl=3, _num_iterations=0)
    pairs = iter([(1.0, 1.0)] * 2 + [(9.0, 0.0)] + [(9.0, 1.0)] * 5)
    monkeypatch.setattr(ness, "online_move", lambda a, y, s: (calls.append("move"), next(pairs))[1])
    for t in range(8):
        state = alg.step(None, state)
    # calls 3 and 6 (however low the ESS is in between), and call 4 follows a move that left a non-finite weight
    assert calls == ["move", "move", "update", "move", "update", "move", "move", "update", "move", "move", "move"]


def test_a_process_group_is_refused():
    from pyfilter_amd.inference import NESS, FixedWidthNESS

    for cls in (NESS, FixedWidthNESS):
        with pytest.raises(NotImplementedError, match="one GPU"):
            cls(object(), 8, priors(), device="cpu", group=object())


def test_robust_var_replaces_the_variance_where_the_iqr_is_not_larger():
    """``jittering.py:51-89``: column 0 has an outlier (IQR^2 < var: replaced), column 1 is two-point (IQR^2 > var: kept)."""
    from pyfilter_amd.inference.ness import robust_var

    x = torch.tensor([[0.0, -1.0], [0.1, -1.0], [0.2, 1.0], [0.3, 1.0], [50.0, 1.0]], dtype=torch.float64)
    w = torch.full((5,), 0.2, dtype=torch.float64)
    mean = (w.unsqueeze(-1) * x).sum(0)
    var = (w.unsqueeze(-1) * (x - mean) ** 2).sum(0)
    # cdf 0.2 .. 1.0: |cdf - 0.25| is least at index 0, |cdf - 0.75| ties at 0.6 / 0.8 up to rounding: take what torch picks
    cdf = w.cumsum(0)
    lo, hi = int((cdf - 0.25).abs().argmin()), int((cdf - 0.75).abs().argmin())
    srt = x.sort(0).values
    iqr2 = ((srt[hi] - srt[lo]) / 1.349) ** 2
    assert iqr2[0] < var[0] and iqr2[1] > var[1]
    torch.testing.assert_close(robust_var(x, w), torch.stack([iqr2[0], var[1]]), rtol=1e-14, atol=0.0)


def test_constant_kernel_takes_a_number_or_a_tensor_and_the_std_is_clamped():
    from pyfilter_amd.inference import ConstantKernel, NonShrinkingKernel

    g = torch.Generator().manual_seed(0)
    x = torch.randn(9, 2, generator=g, dtype=torch.float64)
    w = torch.full((9,), 1 / 9, dtype=torch.float64)
    idx = torch.arange(9).flip(0)
    eps = torch.randn(9, 2, generator=g, dtype=torch.float64)
    a = ConstantKernel(0.25).jitter(x, w, idx, eps)
    b = ConstantKernel(torch.tensor(0.25)).jitter(x, w, idx, eps)
    c = ConstantKernel(torch.tensor([0.25, 0.25])).jitter(x, w, idx, eps)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, x[idx] + 0.25 * eps)
    # every particle agrees: zero variance -> the std is the threshold (the reference's EPS = sqrt(machine epsilon))
    k = NonShrinkingKernel()
    same = torch.ones(9, 2, dtype=torch.float64)
    out = k.jitter(same, w, idx, eps)
    assert torch.equal(k.last_fit[2], torch.full((2,), torch.finfo(torch.float64).eps ** 0.5, dtype=torch.float64))
    assert torch.equal(out, same + k.last_fit[2] * eps)
