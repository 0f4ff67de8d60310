"""The one-column leaf at five workgroups per CU (``pf_fused.hpp: PF_WAVES_LEAF, StepLds``): its residency, and its two smaller LDS
windows where the heads scatter and the window walk are stressed.

The leaf declares ``win`` as the heads of one round plus the dump slots (1 024 + 64 ints) and ``xwin`` as the staged entries
(1 280 floats) - not the searching variants' 2 048 each.  Both are exactly enough only because of how ``inverse_grid_round`` and the
gather use them, so the runs here put the weight of ONE resampling on a few particles scattered over the column:

* most staged cdf entries then own no position of their tile's round, and write their head to a dump slot ``hd[RE .. RE + 63]``;
* a tile whose 1 024 positions fall to heavy particles more than 1 280 entries apart walks on window by window (``next_window``), and
  its ancestors lie beyond what ``xwin`` holds: the ``in_lds`` test must send the gather to global memory.

The data: the sine model's series of ``test_onecol_leaf_gpu.py`` (T = 12, no NaN row) with the observation of the interior step
``S = 5`` displaced by ``DISPLACE[proposal]`` predictive standard deviations (``PRED_STD`` of that file).  The APF resamples step ``S``
on its first-stage weights under that observation.  The displacements were picked with ``oracle/cpu_ref.py`` on the CPU (float64, its
own draws, a run that ends at step ``S``), so that the reference's own ancestors of step ``S`` meet both preconditions with room:

    proposal   displacement   N        distinct ancestors    tiles spanning > 1 280 indices   widest tile
    lgo        200            16 384     215  (1.3 %)          4 of 16                          5 697
    lgo        200            32 768     420  (1.3 %)         11 of 32                          5 782
    bootstrap    6            16 384      76  (0.5 %)          5 of 16                          5 614
    bootstrap    6            32 768     129  (0.4 %)         12 of 32                          4 588

On an MI355X the library's own draws give, in the same order: 271 distinct ancestors (1.65 %), 4 of 16 tiles, widest 5 388; 262 (0.80 %),
7 of 32, 8 939; 71 (0.43 %), 6 of 16, 3 292; 135 (0.41 %), 9 of 32, 4 731 - and 6 resident workgroups per CU on 256 CUs for all four leaves.

(The optimal proposal's first-stage weights are taken under the one-step predictive density, which is flat over the tight cloud an
adapted filter carries: at 25 standard deviations - ``test_degenerate_weights`` - three quarters of the particles still have offspring
at step ``S``; the Bootstrap proposal's are taken under the observation density and collapse onto one particle beyond 12.)

The preconditions are asserted on the GPU's own ancestors, not hoped for: a generic run of a third filter object of the same seed
that ENDS at step ``S`` stores that step's ancestors (the launch writes a kept state), and its first call draws what the first calls
of the two compared objects draw.  Every comparison is ``torch.equal`` on bit patterns, the scaffolding ``test_onecol_leaf_gpu.py``'s."""
import functools

import pytest
import torch

from pyfilter_amd import _lib, ops
from tests.test_onecol_leaf_gpu import (F32, PRED_STD, _assert_leaf_trace, _assert_same, _case, _filter, _leaf_and_generic,
                                        _observations, _run)

pytestmark = pytest.mark.gpu

T_LEN = 12
S = 5
DISPLACE = {"lgo": 200.0, "bootstrap": 6.0}  # predictive standard deviations (the table above)
TILE = 1024    # positions of one step workgroup: 256 lanes x 4
STAGED = 1280  # cdf entries / particles one window stages: 256 x (4 + 1)


@pytest.mark.parametrize("mk", [1, 2])
@pytest.mark.parametrize("proposal", [_lib.PROP_BOOTSTRAP, _lib.PROP_LGO], ids=["bootstrap", "lgo"])
def test_leaf_residency(proposal, mk):
    """Five workgroups of every leaf instantiation fit a CU, and a full-chip launch - 2^20 particles: 1 024 step workgroups and the
    bookkeeper - is resident at once."""
    blocks_per_cu, cus = ops.debug_leaf_residency(proposal, mk)
    print(f"leaf PROP {proposal} MK {mk}: {blocks_per_cu} workgroups per CU on {cus} CUs")
    assert blocks_per_cu >= 5
    assert blocks_per_cu * cus >= (1 << 20) // TILE + 1


@functools.lru_cache(maxsize=None)
def _runs(prop, n):
    """(y, ancestors of step S from a generic run that ends there, leaf-side (planes, trace), generic-side (planes, trace))"""
    case = _case("sine", prop, n, t_len=T_LEN, nan_steps=())
    y = _observations(case, F32)
    y[S] = y[S] + DISPLACE[prop] * PRED_STD["sine"]
    anc = _run(_filter(case, F32), y[:S + 1], True)[0]["ancestors"].reshape(-1).cpu()
    own, gen, _ = _leaf_and_generic(case, y)
    return y, anc, own[0], gen[0]


@pytest.mark.parametrize("n", [16384, 32768])
@pytest.mark.parametrize("prop", ["lgo", "bootstrap"])
def test_scattered_heavy_particles_equal_generic(prop, n):
    y, anc, own, gen = _runs(prop, n)
    assert anc.numel() == n
    tiles = anc.reshape(-1, TILE)
    span = tiles.max(1).values - tiles.min(1).values
    distinct = int(anc.unique().numel())
    print(f"{prop} {n}: step {S} has {distinct} distinct ancestors ({100.0 * distinct / n:.2f} %), {int((span > STAGED).sum())} of "
          f"{tiles.shape[0]} tiles span more than {STAGED} indices, the widest {int(span.max())}")
    assert int(span.max()) > STAGED, "no tile's ancestors reach beyond one staged window: the window walk is not exercised"
    assert 4 * distinct < n, "too many particles have offspring: the dump slots are hardly written"
    _assert_same(own[0], gen[0], f"sine {prop} {n}, step {S} displaced by {DISPLACE[prop]} predictive standard deviations")


@pytest.mark.parametrize("n", [16384, 32768])
@pytest.mark.parametrize("prop", ["lgo", "bootstrap"])
def test_scattered_heavy_particles_take_the_leaf(prop, n):
    """The same runs: every launch but the run's last is a leaf launch (no NaN row: SPEC = 1 throughout), the generic side has none."""
    y, _, own, gen = _runs(prop, n)
    _assert_leaf_trace(own[1], y, "leaf run")
    assert sum(r["LEAF"] for r in own[1]) == T_LEN - 1
    assert all(r["LEAF"] == 0 for r in gen[1]) and [r["step"] for r in gen[1]] == list(range(T_LEN)), gen[1]
