"""The host oracle of the in-kernel random numbers (``tests/philox_ref.py``) without a GPU: Philox4x32-10 against the published
known answers, the address maps of every draw the kernels make are injective, the restatement's draws have the moments they
should, and the INPUT CONDITION of the ancestor checks of ``tests/test_philox_draws_gpu.py`` holds - few resampling positions
within ``delta`` of a cdf entry, for every shape and teacher state those tests use.

The jitter kernel's draws: ``tests/theta_oracle.py`` and ``tests/test_theta_oracle_cpu.py``."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from oracle.cases import build_spec
from tests import philox_cases as PC
from tests import philox_ref as P
from tests.source_registries import streams_in_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyfilter_amd", "csrc")
DTYPES = ("float32", "float64")


# ---- the generator -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", [
    # Random123 kat_vectors, philox4x32-10
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_known_answers(ctr, key, want):
    got = P.philox4x32_10(*[np.array([c], dtype=np.uint64) for c in ctr], *key)
    assert tuple(int(w[0]) for w in got) == want
    # ... and vectorised: the same answer in every lane of a broadcast call
    got = P.philox4x32_10(np.full(5, ctr[0], dtype=np.uint64), ctr[1], ctr[2], ctr[3], *key)
    assert all((w == v).all() for w, v in zip(got, want))


def test_call_splits_seed_and_counter_into_words():
    seed, ctr = PC.SEED_HIGH, np.array([(7 << 32) | 9], dtype=np.uint64)
    want = P.philox4x32_10(9, 7, 5, 3, seed & 0xFFFFFFFF, seed >> 32)
    got = P.call(seed, 3, 5, ctr)
    assert all(int(a[0]) == int(b) for a, b in zip(got, want))


def test_word_to_number():
    top = np.array([0xFFFFFFFF], dtype=np.uint64)
    zero = np.array([0], dtype=np.uint64)
    assert P.u01(zero)[0] == 0.0 and P.u01(top)[0] == 1.0 - 2.0 ** -24
    assert P.u01_open0(zero)[0] == 2.0 ** -24 and P.u01_open0(top)[0] == 1.0
    assert P.u01_d(zero, zero)[0] == 0.0 and P.u01_d(top, top)[0] == 1.0 - 2.0 ** -53
    assert P.u01_open0_d(zero, zero)[0] == 2.0 ** -53 and P.u01_open0_d(top, top)[0] == 1.0
    assert P.u01_d(np.array([1], dtype=np.uint64), zero)[0] == 2.0 ** 32 / 2.0 ** 64  # the FIRST word is the high one
    assert P.u01(np.array([0x100], dtype=np.uint64))[0] == 2.0 ** -24             # the low 8 bits are dropped


# ---- stream words ------------------------------------------------------------------------------------------------------------
def test_stream_words_are_those_of_the_sources_and_distinct():
    """The one enum of ``pf_philox.hpp`` (a ``PF_STREAM_*`` defined anywhere else fails the parse) against ``philox_ref.STREAMS``."""
    src = streams_in_sources()
    assert src == P.STREAMS and len(src) == 11, (src, P.STREAMS)
    with open(os.path.join(CSRC, "pf_philox.hpp")) as f:
        flags = set(re.findall(r"stream \| (0x[0-9a-fA-F]+)u", f.read()))
    assert flags == {hex(P.EXP_FLAG)}, flags
    words = list(src.values()) + [src["MULTINOMIAL"] | P.EXP_FLAG]
    assert len(set(words)) == len(words), words


# ---- the step kernel's tilings at the shapes of the GPU tests ------------------------------------------------------------------
def test_step_shapes_have_the_tilings_they_are_chosen_for():
    """One tile of one round; one tile of four scalar rounds; several tiles with a ragged last one; tiles of several rounds - read from
    the geometry rule (``make_geom``, restated by ``philox_cases.step_geometry`` on the constants parsed from the sources)."""
    def const(name):
        for f in ("pf_host.hpp", "pf_device.hpp"):
            with open(os.path.join(CSRC, f)) as src:
                m = re.search(rf"#define\s+{name}\s+(\d+)", src.read())
            if m:
                return int(m.group(1))
        raise AssertionError(name)

    with open(os.path.join(CSRC, "pf_host.hpp")) as src:
        body = src.read()
    assert "int min_r = (g.vec == 4) ? 1 : 4;" in body and "g.vec = (N % 4 == 0) ? 4 : 1;" in body, "make_geom changed: restate it"
    assert const("PF_TARGET_WGS") == 1024
    for (n, b, target), want in zip(PC.STEP_SHAPES, PC.STEP_TILINGS):
        assert PC.step_geometry(n, b, target, block=const("PF_BLOCK"), max_tiles=const("PF_MAX_TILES")) == want, (n, b, target)


# ---- address maps ------------------------------------------------------------------------------------------------------------
def _words(stream, step, address, dtype):
    """The 32-bit words ``(stream word, step, call, word)`` behind draws at ``address = (call, slot)`` arrays - the address maps are
    ``philox_ref``'s own (``normal_address``, ``exponential_address``, ``uniform_address``, ``slot_words``): the ones its draws, and so
    the GPU tests, go through."""
    at, slot = (np.asarray(a).ravel() for a in address)
    return [(stream, step, int(c), w) for c, k in zip(at, slot) for w in P.slot_words(k, dtype)]


def _normal_words(stream, step, elem, d, dtype):
    return _words(stream, step, P.normal_address(elem, d, dtype), dtype)


def _uniform_words(stream, step, elem, dtype):
    return _words(stream, step, P.uniform_address(elem, dtype), dtype)


def _exp_words(step, elem, dtype):
    return _words(P.STREAMS["MULTINOMIAL"] | P.EXP_FLAG, step, P.exponential_address(elem, dtype), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [1, 2, 3])
def test_address_maps_are_injective(d, dtype):
    """No two consumers - particles, filters, state components, candidates, steps, streams - of a small run share a 32-bit word.
    (Box-Muller: the two normals of a pair share the pair's words BY DESIGN - each is counted as owning its share,
    ``philox_ref.slot_words``.)"""
    n, b, m, maxo = 13, 3, 5, (1 if d == 1 else 3)
    S = P.STREAMS
    cols = np.arange(b * n)
    words = []
    for step in (0, 1, 7):
        words += _normal_words(S["NORMAL"], step, cols, d, dtype)                      # the moves' normals
        words += _uniform_words(S["UNIFORM"], step, np.arange(b), dtype)               # the systematic offsets
        words += _uniform_words(S["MULTINOMIAL"], step, cols, dtype)                   # the stand-alone multinomial's uniforms
        words += _exp_words(step, np.concatenate([cols, b * n + np.arange(b)]), dtype)  # spacings and the filters' tail spacings
        words += _uniform_words(S["SMOOTH"], step, cols, dtype)                        # backward draws
        words += _normal_words(S["NESTED_Z"], step, (cols[:, None] * m + np.arange(m)).ravel(), d, dtype)
        words += _uniform_words(S["NESTED_PICK"], step, cols, dtype)
        words += _normal_words(S["FORECAST_Z"], step, cols, d, dtype)
        words += _normal_words(S["FORECAST_E"], step, cols, maxo, dtype)
    # the initial sample: D of the 4 numbers of an element, plane group g (three planes each) at step word g
    for group in (0, 1, 2):
        words += _normal_words(S["INIT"], group, cols, 4, dtype)
    assert len(set(words)) == len(words), f"{len(words) - len(set(words))} words are read twice"


@pytest.mark.parametrize("dtype", DTYPES)
def test_draws_of_different_addresses_differ(dtype):
    """... and by VALUE: the restatement's draws over (filter, particle, component), (stream), (step) are all different numbers."""
    n, b = 257, 3
    elem = np.arange(n * b, dtype=np.uint64)
    for d in (1, 2, 3):
        z = np.concatenate([P.normals(PC.SEED_LOW, s, t, elem, d, dtype).ravel() for s in (0, 2, 6, 8, 9) for t in (0, 1)])
        assert len(np.unique(z)) == z.size
    e = np.concatenate([P.exponentials(PC.SEED_LOW, t, np.arange(n * b + b, dtype=np.uint64), dtype) for t in (0, 1)])
    assert len(np.unique(e)) == e.size
    if dtype == "float64":  # (24-bit uniforms repeat by chance: a birthday bound, not an addressing statement)
        u = np.concatenate([P.uniform(PC.SEED_LOW, s, t, elem, dtype) for s in (1, 3, 5, 7) for t in (0, 1)])
        assert len(np.unique(u)) == u.size


# ---- sanity of the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_moments_of_the_restatement(dtype):
    n = 100_000
    elem = np.arange(n, dtype=np.uint64)
    for seed in (PC.SEED_LOW, PC.SEED_HIGH):
        z = P.normals(seed, 0, 3, elem, 1, dtype)[:, 0]
        assert abs(z.mean()) < 5.0 / np.sqrt(n) and abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / n)
        e = P.exponentials(seed, 3, elem, dtype)
        assert (e > 0).all() and abs(e.mean() - 1.0) < 5.0 / np.sqrt(n) and abs(e.var() - 1.0) < 5.0 * np.sqrt(8.0 / n)  # var of (E-1)^2 = 8
        u = P.uniform(seed, 1, 3, elem, dtype)
        assert (u >= 0).all() and (u < 1).all() and abs(u.mean() - 0.5) < 5.0 * np.sqrt(1.0 / 12.0 / n)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,b", PC.fused_shapes())
def test_positions_are_increasing_inside_the_unit_interval(n, b, dtype):
    for k in range(b):
        p, pr = P.multinomial_positions(PC.RUN_SEED, 1, k, n, b, dtype)
        assert p.shape == (n,) and (np.diff(p) > 0).all() and p[0] > 0 and p[-1] < 1
        assert (np.diff(pr) >= 0).all() and np.abs(pr - p).max() <= (2.0 ** -24 if dtype == "float32" else 0.0)
    # mutation "the tail spacing dropped from the total": the last position is then 1 - not inside (0, 1)
    e = P.exponentials(PC.RUN_SEED, 1, np.arange(n, dtype=np.uint64), dtype)
    assert abs(P.positions_from_spacings(e, 0.0, dtype)[0][-1] - 1.0) < 1e-12 < 1.0 - p[-1]


def test_valid_ancestor_is_searchsorted_with_slack():
    cdf = P.cdf64(np.array([0.1, 0.0, 0.0, 0.4, 0.5]))  # 0.1 0.1 0.1 0.5 1
    p = np.array([0.05, 0.1, 0.1000001, 0.3, 0.5, 0.99])
    exact = np.searchsorted(cdf, p, side="left")
    assert exact.tolist() == [0, 0, 3, 3, 3, 4]
    assert P.valid_ancestor(exact, p, cdf, 0.0).all()
    # a flat stretch (particles without weight): its later entries pass only for a position within delta of the stretch's value
    assert not P.valid_ancestor(np.array([1, 2]), np.array([0.1, 0.1]), cdf, 0.0).any()
    assert P.valid_ancestor(np.array([1, 2]), np.array([0.1, 0.1]), cdf, 1e-3).all()
    assert not P.valid_ancestor(np.array([1, 2, 1, 2]), np.array([0.102, 0.102, 0.098, 0.098]), cdf, 1e-3).any()
    # one entry off is valid exactly where the position is within delta of the entry between the two
    off = np.array([3, 3, 0, 4, 4, 3])
    assert P.valid_ancestor(off, p, cdf, 1e-6).tolist() == [False, True, True, False, True, False]
    assert P.valid_ancestor(np.array([5, -1]), np.array([0.99, 0.05]), cdf, 1.0).tolist() == [False, False]  # out of range
    assert P.near_boundary(p, cdf, 1e-6).tolist() == [False, True, True, False, True, False]


# ---- the input condition of the GPU ancestor checks -----------------------------------------------------------------------------
TORCH_DT = {"float32": torch.float32, "float64": torch.float64}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,b", PC.fused_shapes())
def test_few_positions_near_a_cdf_entry_teacher_weights(n, b, dtype):
    """First move (step word 0) from the teacher weights: softmax of ``2 randn``, filter 0 half-zero."""
    dt = TORCH_DT[dtype]
    W = PC.weights64(PC.teacher_logw(n, b, dt))
    shares = PC.near_share(PC.RUN_SEED, 0, W, dt, PC.DELTA[dt])
    print(f"philox-near: teacher {n}x{b} {dtype} share within {PC.DELTA[dt]:g} of a cdf entry:", ["%.4f" % s for s in shares])
    assert max(shares) <= PC.NEAR_SHARE, shares


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,b", PC.fused_shapes())
@pytest.mark.parametrize("model", PC.MODELS)
def test_few_positions_near_a_cdf_entry_second_move(model, n, b, dtype):
    """Second move of a two-move run (step word 1): the weights are the observation densities of the first move's particles - here
    the oracle's own first move (the GPU test states the same condition on the weights it meets)."""
    dt = TORCH_DT[dtype]
    case = PC.case_of(model, "sisr", "bootstrap", n, b)
    spec = build_spec(case, torch.float64)
    y = PC.observations(case, dt).double()
    x, logw = PC.teacher(case, dt)
    _, x1 = PC.oracle_sisr_bootstrap_move(case, dt, x, logw, PC.RUN_SEED, 0)
    from oracle import models as M

    w1 = M.obs_log_prob(spec, y[0], x1).to(dt)
    shares = PC.near_share(PC.RUN_SEED, 1, PC.weights64(w1), dt, PC.DELTA[dt])
    assert max(shares) <= PC.NEAR_SHARE, shares


@pytest.mark.parametrize("n,b", PC.fused_shapes())
@pytest.mark.parametrize("model", ["sine", "rw2d"])
def test_few_positions_near_a_cdf_entry_apf_first_stage(model, n, b):
    """float64 APF + optimal proposal: the cdf of the first-stage weights ``pre_weight + log w`` (``cpu_ref.apf_step``), delta 1e-11."""
    case = PC.case_of(model, "apf", "lgo", n, b)
    spec = build_spec(case, torch.float64)
    y = PC.observations(case, torch.float64)
    x, logw = PC.teacher(case, torch.float64)
    rw = cpu_ref.lgo_pre_weight(spec, y[0], x) + logw
    shares = PC.near_share(PC.RUN_SEED, 0, PC.weights64(rw), torch.float64, PC.DELTA_APF)
    assert max(shares) <= PC.NEAR_SHARE, shares


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,b", PC.MULTINOMIAL_SHAPES)
def test_few_uniforms_near_a_cdf_entry_stand_alone_multinomial(n, b, dtype):
    dt = TORCH_DT[dtype]
    W = PC.weights64(PC.teacher_logw(n, b, dt))
    for k in range(b):
        u = P.uniform(PC.SEED_LOW, P.STREAMS["MULTINOMIAL"], 5, k * n + np.arange(n, dtype=np.uint64), dtype)
        assert P.near_boundary(u, P.cdf64(W[:, k].numpy()), PC.DELTA[dt]).mean() <= PC.NEAR_SHARE


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,b", [(333, 3), (4100, 2), PC.CLUSTER_SHAPE])
def test_few_grid_positions_near_a_cdf_entry_systematic_offset(n, b, dtype):
    dt = TORCH_DT[dtype]
    W = PC.weights64(PC.teacher_logw(n, b, dt))
    for k in range(b):
        u = P.uniform(PC.RUN_SEED, P.STREAMS["UNIFORM"], 0, np.array([k], dtype=np.uint64), dtype)[0]
        grid = (np.arange(n) + u) / n
        assert P.near_boundary(grid, P.cdf64(W[:, k].numpy()), PC.DELTA[dt]).mean() <= PC.NEAR_SHARE
