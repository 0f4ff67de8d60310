"""``"ffbs-mh"`` without a GPU: the entry points are declared, the host oracle of ``tests/smoothing_mh_oracle.py`` targets the law
backward simulation targets and degenerates to ancestor tracing at K = 0, and the float32 oracle stays within the GPU bars of
``tests/test_smoothing_mh_gpu.py`` of the float64 oracle on every case those tests run."""
import os
import re

import pytest
import torch

from oracle import cpu_ref
from tests import linmat_smoothing_cases as lsc
from tests import philox_ref as P
from tests import smoothing_cases as sc
from tests import smoothing_mh_oracle as mh
from tests.helpers import DT
from tests.source_registries import streams_in_sources, trace_codes_in_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRAW_CASES, IDS = mh.DRAW_CASES, mh.DRAW_IDS
WITH_DRAWS = [c for c in DRAW_CASES if c[3] > 1]  # (S = 1 has no backward draw)


def test_entry_points_are_declared():
    """Header, ``_lib.EXPORTS``, the launch-trace name, and a Philox stream word no other draw of the library uses."""
    from pyfilter_amd import _lib, ops

    assert "pf_smooth_mh" in _lib.EXPORTS and "pf_smooth_mh_workspace_bytes" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "pf_amd.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"int pf_smooth_mh\(const pf_model\* model,", header) and "int pf_smooth_mh_workspace_bytes(" in header
    assert "#define PF_ABI_VERSION 4" in header and _lib.ABI_VERSION == 4
    codes = trace_codes_in_sources()
    assert codes == {"FFBS_LINEAR": 20, "SCORE_LINEAR": 21, "SMOOTH_MH": 22}
    assert ops.TRACE_ENTRY == {codes["FFBS_LINEAR"]: "pf_smooth_ffbs_linear", codes["SCORE_LINEAR"]: "pf_path_score_linear",
                               codes["SMOOTH_MH"]: "pf_smooth_mh"}
    streams = streams_in_sources()
    stream = streams.pop("SMOOTH_MH")
    assert stream == 10 == mh.PHILOX_STREAM == P.STREAMS["SMOOTH_MH"]
    assert stream not in streams.values() and stream != (streams["MULTINOMIAL"] | P.EXP_FLAG)
    with open(os.path.join(ROOT, "pyfilter_amd", "csrc", "pf_kernels.hip")) as f:
        assert '#include "pf_smooth_mh.hpp"' in f.read()


@pytest.mark.parametrize("model", ["sine", "rw2d"])
def test_oracle_targets_the_backward_categorical(model):
    """4 096 chains from one x+, 16 live candidates, random (mostly dead) starts: at K = 64 the picks follow the categorical of
    ``cpu_ref.ffbs_backward_step`` (chi-square over the live candidates with an expected count >= 5 below 60); at K = 8 on the same
    inputs they do not - the test can tell a chain that has not mixed."""
    got = {}
    for k in (64, 8):
        c = mh.law_case(model, torch.float64, k)
        picks = mh.oracle_pass(c, torch.float64)[0]["pick"][:, 0]
        got[k] = mh.law_chi2(c, picks)
        print(f"smoothing-mh-law: oracle {model} K={k}: chi2 {got[k][0]:.1f} over {got[k][1]} bins")
    assert got[64][0] < mh.CHI2_BAR, got
    assert got[8][0] > mh.CHI2_BAR, got


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("model,n,b,s", [("sine", 257, 2, 3), ("rw2d", 300, 1, 4), (4, 257, 2, 3)])
def test_no_rounds_is_ancestor_tracing(model, n, b, s, dt):
    """K = 0: the pass is ``cpu_ref.smooth_fl`` over the history, read at ``idx_last``."""
    c = mh.case(model, n, b, s, DT[dt], 0)
    out, idx = mh.paths_of(c, mh.oracle_pass(c, torch.float64))
    fl = cpu_ref.smooth_fl(c.h.x, list(c.anc.unbind(0)))  # (S, N, B, [D]): the lines of the last state's particles
    want = torch.stack([sc.gather(fl[t], c.idx_last) for t in range(s)], 0)
    assert torch.equal(out, want)
    walk = c.idx_last
    for t in range(s - 2, -1, -1):
        walk = c.anc[t + 1].gather(0, walk)
        assert torch.equal(idx[t], walk)


@pytest.mark.parametrize("model,n,b,s,k", WITH_DRAWS, ids=[i for c, i in zip(DRAW_CASES, IDS) if c[3] > 1])
def test_float32_oracle_against_the_float64_oracle(model, n, b, s, k):
    """The conditions of the GPU bars, on the oracle alone: the float32 oracle, teacher-forced with the float64 oracle's pass,
    differs from it in at most 1e-3 of a case's chains, each within the float32 bars (4 x its own cdf / l' - l error)."""
    c = mh.case(model, n, b, s, torch.float32, k)
    ref = mh.oracle_pass(c, torch.float64)
    out, idx = mh.paths_of(c, ref)
    low = mh.oracle_pass(c, torch.float32, forced=lambda t: (out[t], idx[t]))
    delta_p, delta_a = mh.deltas(c, ref, low)
    picks = torch.stack([r["pick"] for r in low] + [c.idx_last], 0)
    bad, total, worst_p, worst_a = mh.compare(c, picks, ref, delta_p, delta_a, mh.label(model, n, b, s, k))
    print(f"smoothing-mh-parity: float32 oracle {mh.label(model, n, b, s, k)}: {bad} of {total} chains differ "
          f"(margins {worst_p:.3e} / {worst_a:.3e}), delta_p {delta_p:.3e}, delta_a {delta_a:.3e}")


def test_philox_uniforms_of_the_stated_key_are_in_range():
    """``philox_uniforms``: call (b N + j) K + r of (seed, stream 10, step t), slots 0 and 1 - shape, range and distinct rounds."""
    from tests.smoothing_mh_oracle import philox_uniforms

    for dtype in (torch.float32, torch.float64):
        u = philox_uniforms(7, 3, 2, 5, 2, dtype)
        assert u.shape == (2, 2, 2, 5, 2) and u.dtype == dtype and bool((u >= 0).all()) and bool((u < 1).all())
        assert u.unique().numel() == u.numel()


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("model", ["sine", 4])
def test_oracle_fallback_is_the_last_candidate_of_positive_mass(model, dt):
    """``fallback_case``: 100 trailing candidates without mass, ``u1 = 1`` for chains 0 .. 9 - the oracle takes the fallback there,
    and only there, and proposes candidate N - 101; ``u1 = 1 - eps`` (chains 10 .. 19) reaches the same candidate by the search."""
    n, b, s, k = 600, 2, 3, 2
    c = mh.fallback_case(model, n, b, s, DT[dt], k)
    u = c.u.clone()
    u[:, :, 0, 10:20] = 1.0 - torch.finfo(DT[dt]).eps
    c = c.edited(u=u)
    last = n - 1 - mh.TRAILING_DEAD
    for r in mh.oracle_pass(c, torch.float64):
        assert bool(r["fallback"][:, :10].all()) and not bool(r["fallback"][:, 10:].any())
        assert bool((r["prop"][:, :20] == last).all()) and bool((r["pick"][:20] == last).all())
        assert bool((r["pick"] <= last).all())
